"""Free-path flights at their edges without a GPU: the restatement (tests/free_path_cases.py) reaches the edge every case of
tests/free_path_edge_cases.py is built for, and no ray's facet sequence hinges on the rounding of a hit point (so
test_gpu_free_path_edges.py compares every ray).  Then nk_exp's arithmetic restated step by step (nk_device.h: every step of it is
a fused multiply-add, one rounding -- nk_fma_c is v_fma_f64 --, a product, a rint or an ldexp): what it returned far below its
tested range before it clamped its argument, and that it returns +0 there now."""
import math
from fractions import Fraction

import numpy as np
import pytest

import free_path_cases as FC
import free_path_edge_cases as E


def ends(r):
    return np.bincount(r['ray_end'].ravel(), minlength=5).tolist()


@pytest.mark.parametrize('name', sorted(E.CASES))
def test_sizes_and_sequences(name):
    """The sizes the suite allows itself, finite inputs (but the NaN lifetime of 'dead'), and the same facets with fused and unfused
    hit points on every ray: nothing is left out of a comparison."""
    inp, r = E.inputs(name), E.run(name)
    assert inp['modes'].shape[0] <= 8 and inp['n'] <= 130 and 0 < (inp['max_segments'] or 10 ** 9) <= 64
    assert r['ray_segments'].max() <= 64
    assert np.isfinite(inp['x0']).all() and inp['x0'].shape == (inp['modes'].shape[0], inp['n'], 3)
    t = inp['tau']
    assert np.isfinite(t[t > 0]).all()
    assert E.left_out_share(name) == 0.0 <= FC.MAX_OTHER_SEQUENCE
    assert np.array_equal(r['ray_end'], E.run(name, fused=False)['ray_end'])


@pytest.mark.parametrize('name', E.MISSES)
def test_misses(name):
    inp, r = E.inputs(name), E.run(name)
    out = inp['outside']
    assert out.sum() == 32 and not out[:32].any()                       # half the lanes of the wave
    tc, fc = E.first_cast(inp['ct'], inp['modes'], inp['x0'])
    assert (fc[:, out] < 0).all() and (fc[:, ~out] >= 0).all()
    b = E.bounds(inp['ct'])
    x = inp['x0']
    beyond = ((x < b[0]) | (x > b[1])).any(axis=2)
    assert np.array_equal(beyond, np.broadcast_to(out, beyond.shape))
    assert (r['ray_end'][:, out] == 3).all() and (r['ray_segments'][:, out] == 1).all() and not (r['ray_end'][:, ~out] == 3).any()
    assert r['report']['missed'] == 6 * 32
    v, tau = FC.group_vel(inp['ct'])[inp['modes']], inp['tau'][inp['modes']]
    assert np.array_equal(r['ray_D'][:, out], np.broadcast_to((tau[:, None] * v)[:, None, :], (6, 32, 3)))
    assert np.array_equal(r['ray_T'][:, out], np.broadcast_to(tau[:, None], (6, 32)))
    if name == 'misses_ttp':                                            # every wall is flown away from
        ax = [int(np.nonzero(beyond_axis)[0][0]) for beyond_axis in ((x[:, 63] < b[0]) | (x[:, 63] > b[1]))]
        assert sorted(set(ax)) == [0, 1, 2]


def test_seam():
    inp, r = E.inputs('seam'), E.run('seam')
    a = inp['tc'] / inp['tau'][inp['modes']]                            # as the restatement computes it
    assert (a[inp['side'] == 0] == 0.125).all() and (a[inp['side'] == 1] > 0.125).all() and (a[inp['side'] == 2] < 0.125).all()
    assert np.array_equal(a[inp['side'] == 1], [np.nextafter(0.125, 1.0)] * 2) and (a[inp['side'] == 2] >= 0.125 - 2.0 ** -55).all()
    assert np.array_equal(np.bincount(inp['side']), [2, 2, 2])
    assert (r['ray_end'] == 1).all() and (r['ray_segments'] == 1).all()            # every ray flies to a reservoir
    assert (inp['x0'] == inp['x0'][:, :1]).all()


def test_tiny_tau():
    inp, r = E.inputs('tiny_tau'), E.run('tiny_tau')
    tau, v = inp['tau'][inp['modes']], FC.group_vel(inp['ct'])[inp['modes']]
    assert np.array_equal(tau, E.TINY * 2) and (tau > 0).all()
    tc, fc = E.first_cast(inp['ct'], inp['modes'], inp['x0'])
    with np.errstate(over='ignore'):
        a = tc / tau[:, None]
    # (first flights of 0.1 .. 10 ps in this box: a of 1e17 .. 1e19, 1e59 .. 1e61, 1e300 .. 1e302 and inf)
    assert a[0].min() > 1e16 and a[0].max() > 1e18 and a[1].min() > 1e58 and a[2].min() > 1e299 and np.isinf(a[3]).all()
    # W = 0 after the first segment: nothing is left for the reservoirs, the walls or w_left
    assert (r['ray_segments'] == 1).all() and (r['ray_end'][inp['along']] == 0).all() and set(np.unique(r['ray_end'])) == {0, 1}
    for k in ('hits', 'p_res', 'p_wall', 'w_left'):
        assert not r[k].any(), k
    assert np.array_equal(r['p_int'], [64.0] * 8)
    assert np.array_equal(r['ray_D'], np.broadcast_to((tau[:, None] * v)[:, None, :], (8, 64, 3)))
    assert np.array_equal(r['ray_T'], np.broadcast_to(tau[:, None], (8, 64)))
    assert all(np.isfinite(r[k]).all() for k in FC.MODE_KEYS + ('ray_D', 'ray_T'))


@pytest.mark.parametrize('name', ['huge_tau_ttp', 'huge_tau_wire72'])
def test_huge_tau(name):
    """tau = 2^900: g = a, e = 1, W stays 1 -- the ballistic limit, D = sum of tc v over the segments."""
    inp, r = E.inputs(name), E.run(name)
    assert (inp['tau'][inp['modes']] == 2.0 ** 900).all()
    v = FC.group_vel(inp['ct'])
    tc, fc = E.first_cast(inp['ct'], inp['modes'], inp['x0'])
    one = r['ray_segments'] == 1
    assert one.any() and np.isfinite(r['ray_D']).all()
    flown = tc[..., None] * v[inp['modes']][:, None, :]
    assert np.allclose(r['ray_D'][one], flown[one], rtol=1e-14, atol=0) and np.allclose(r['ray_T'][one], tc[one], rtol=1e-14, atol=0)
    assert np.array_equal(r['hits'], r['ray_segments'].sum(axis=1))                 # W = 1 at every hit
    if name == 'huge_tau_ttp':
        assert ends(r) == [0, 192, 0, 0, 192] and np.array_equal(r['w_left'], [64.0] * 3 + [0.0] * 3)


@pytest.mark.parametrize('name', ['dead_ttp', 'dead_wire72'])
def test_dead(name):
    inp, r = E.inputs(name), E.run(name)
    d = inp['dead']
    t = inp['tau'][inp['modes']]
    assert t[0] == 0.0 and t[1] == -1.0 and np.isnan(t[2]) and t[3] > 0
    assert not r['ray_end'][d].any() and not r['ray_segments'][d].any() and not r['ray_T'][d].any() and not r['ray_D'][d].any()
    assert np.array_equal(r['p_int'][d], [64.0] * 3) and np.array_equal(r['T'][d], [0.0] * 3)
    assert (r['ray_segments'][~d] >= 1).all() and r['report']['casts'] == r['ray_segments'][~d].sum()


def test_limits():
    one, small, seg = E.run('wmin_one'), E.run('wmin_smallest'), E.run('one_segment')
    # w_min = 1: a ray that goes on ends after its first segment with code 0 and what is left of its weight, e
    inp = E.inputs('wmin_one')
    tc, fc = E.first_cast(inp['ct'], inp['modes'], inp['x0'])
    assert (one['ray_segments'] == 1).all() and set(np.unique(one['ray_end'])) == {0, 1}
    e = np.exp(-tc / inp['tau'][inp['modes']][:, None])
    assert np.array_equal(one['w_left'], np.where(one['ray_end'] == 0, e, 0.0).sum(axis=1)) and (e < 1.0).all()
    assert ends(one) == [326, 58, 0, 0, 0]
    # w_min = 5e-324: no ray is cut by its weight
    assert ends(small) == [0, 192, 0, 0, 192] and small['ray_segments'].max() == 64 and small['report']['capped'] == 192
    # max_segments = 1
    assert ends(seg) == [0, 58, 0, 0, 326] and (seg['ray_segments'] == 1).all()
    assert np.array_equal(seg['ray_end'] == 1, one['ray_end'] == 1)


def test_shapes():
    """n = 1, 63, 65: a single lane, one idle lane, a second pass that holds one ray; more than one way to end in each."""
    assert sorted(E.SHAPES) == sorted('n%d_%s' % (n, b) for n in (1, 63, 65) for b in ('ttp', 'wire72'))
    for name in E.SHAPES:
        r, n = E.run(name), E.inputs(name)['n']
        assert r['ray_end'].shape == (6, n) and name.startswith('n%d_' % n)
        assert len(set(np.unique(r['ray_end']))) >= 2 and (r['ray_segments'] >= 1).all()


@pytest.mark.parametrize('base', ['ttp', 'wire72'])
def test_columns(base):
    """The columns die in different orders; a miss ends every live column at once; a dead column never starts."""
    inp = E.inputs('misses_' + base)
    taus = E.column_taus(base)
    assert taus.shape == (4, inp['ct']['M']) and np.array_equal(taus[3], FC.lifetimes(inp['ct']))
    cols = [E.run_column(base, c) for c in range(4)]
    out = inp['outside']
    seg = np.stack([c['ray_segments'] for c in cols])
    dead = ~(taus[1][inp['modes']] > 0)
    assert dead.all() and not seg[1].any() and not cols[1]['ray_end'].any()
    for c in (0, 2, 3):
        assert (cols[c]['ray_end'][:, out] == 3).all() and (seg[c][:, out] == 1).all()
    assert (seg[0] == 1).all() and (seg[0] <= seg[3]).all() and (seg[3] <= seg[2]).all()
    if base == 'ttp':                                                   # (the wire's rays end at their first facet)
        assert (seg[0] < seg[3]).any()
    assert np.array_equal(cols[3]['ray_end'], E.run('misses_' + base)['ray_end'])


def test_cell_planes():
    from nanokappa_amd import field as FD
    inp, r = E.inputs('cell_planes'), E.run('cell_planes')
    lo, h, n = inp['lo'], inp['h'], inp['n_cells']
    assert tuple(n) == (7, 3, 2) and h[0] == 200.0 / 7.0
    x = inp['x0'].reshape(-1, 3)
    for a in range(3):                                                  # every plane of every axis, lo and the upper boundary too
        planes = lo[a] + np.arange(n[a] + 1) * h[a]
        assert np.isin(x[:, a], planes).all() and np.isin(planes, x[:, a]).all()
    c, out = FD.cell_index(x, lo, h, n)
    hi = E.bounds(inp['ct'])[1]
    assert np.array_equal(lo + np.asarray(n) * h, hi)                   # the last plane is the box's upper boundary, exactly
    # a point on the upper boundary lands in the last cell.  In y and z the rule's floor((x - lo) (1 / h)) gives n there and the point
    # is counted as clamped; in x, 200 fl(1 / (200 / 7)) = 6.999999999999999 and it is in the last cell by the rule itself
    assert all((c[x[:, a] == hi[a], a] == n[a] - 1).all() for a in range(3))
    assert (200.0 - lo[0]) * (1.0 / h[0]) < 7.0
    assert np.array_equal(out, (x[:, 1:] == hi[1:]).any(axis=1)) and out.sum() == 2 * (96 - 8 * 3 * 2)
    for a in range(3):                                                  # an interior plane belongs to the cell above it
        i = np.rint((x[:, a] - lo[a]) / h[a]).astype(int)
        assert np.array_equal(c[:, a], np.minimum(i, n[a] - 1))
    assert r['report']['missed'] == 108 and (r['ray_end'] == 1).sum() == 84         # rays on a wall that fly outwards miss


# ------------------------------------------------------------------------------------------- nk_exp, step by step
def fma(a, b, c):
    """a b + c with one rounding, exactly: rational arithmetic on the finite path, IEEE's rules for the rest."""
    if not (math.isfinite(a) and math.isfinite(b)):
        return a * b + c
    if not math.isfinite(c):
        return c
    s = Fraction(a) * Fraction(b) + Fraction(c)
    if s == 0:
        return a * b + c if (a == 0.0 or b == 0.0) else 0.0             # (an exact cancellation gives +0)
    try:
        return float(s)
    except OverflowError:
        return math.inf if s > 0 else -math.inf


EXP_C = (2.08767569878681e-09, 2.505210838544172e-08, 2.755731922398589e-07, 2.7557319223985893e-06, 2.48015873015873e-05,
         1.984126984126984e-04, 0.001388888888888889, 0.008333333333333333, 0.041666666666666664, 0.16666666666666666, 0.5, 1.0, 1.0)


def nk_exp(x, clamp):
    """nk_device.h's nk_exp on the host; clamp: with its first statement, x = x < -800 ? -800 : x."""
    if clamp and x < -800.0:
        x = -800.0
    k = float(np.rint(x * 1.4426950408889634))
    r = fma(-k, 6.93147180369123816490e-01, x)
    r = fma(-k, 1.90821492927058770002e-10, r)
    p = 1.6059043836821613e-10
    for c in EXP_C:
        p = fma(p, r, c)
    kc = -2000.0 if k < -2000.0 else (2000.0 if k > 2000.0 else k)
    if not math.isfinite(p):
        return p
    try:
        return math.ldexp(p, 0 if math.isnan(kc) else int(kc))
    except OverflowError:
        return math.copysign(math.inf, p)


def test_nk_exp_restated_in_range():
    """The restatement is nk_exp's: within 1 ulp of exp on its tested range (test_gpu_scalar_math.py holds the device to the same),
    and the clamp changes no bit at or above -800."""
    rng = np.random.default_rng(5)
    xs = np.concatenate((rng.uniform(-745.0, 700.0, 400), rng.uniform(-40.0, 0.0, 400), [0.0, -0.125, -800.0, -745.2, -750.0, 709.0]))
    for x in xs:
        x = float(x)
        y = nk_exp(x, True)
        assert y == nk_exp(x, False) and not math.copysign(1.0, y) < 0
        if x > -700.0:
            want = math.exp(x)
            assert abs(y - want) <= 1.5 * np.spacing(want), x         # (1 ulp of the exact value, half an ulp of libm's rounding)


def test_nk_exp_far_below_its_range():
    """Without the clamp: +0 down to -1e17, then -0.0, a tiny negative number, +inf, -inf and NaN where exp is 0.  With it: +0 with
    the sign bit clear everywhere, and NaN for NaN."""
    plus0, minus0 = [-745.2, -750.0, -1e3, -1e4, -1e10, -1e17], [-1e18, -1e20, -1e30, -1e38]
    for x in plus0:
        y = nk_exp(x, False)
        assert y == 0.0 and math.copysign(1.0, y) > 0, x
    for x in minus0:
        y = nk_exp(x, False)
        assert y == 0.0 and math.copysign(1.0, y) < 0, x
    y = nk_exp(-1e40, False)
    assert -1e-301 < y < -1e-303, y
    for x in (-1e45, -1e60, -1e300):
        assert nk_exp(x, False) == math.inf, x
    assert nk_exp(-1e100, False) == -math.inf
    assert math.isnan(nk_exp(-math.inf, False))
    # 1 - e in nk_fl_decay: -inf or +inf from a positive lifetime below about tc 1e-45
    assert 1.0 - nk_exp(-1e45, False) == -math.inf and 1.0 - nk_exp(-1e100, False) == math.inf
    for x in plus0 + minus0 + [-800.0, np.nextafter(-800.0, -np.inf), -1e40, -1e45, -1e60, -1e100, -1e300, -1.7976931348623157e308, -math.inf]:
        y = nk_exp(float(x), True)
        assert y == 0.0 and math.copysign(1.0, y) > 0, x
    assert math.isnan(nk_exp(math.nan, True)) and nk_exp(710.0, True) == math.inf
