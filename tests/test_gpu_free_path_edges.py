"""Free-path flights on the GPU at their edges (tests/free_path_edge_cases.py; k_free_paths<GEOM, MAP>, k_free_columns<GEOM, KT>, the
flight of nk_flight.h, nk_free_refuse) against the CPU restatement: rays that miss, lifetimes of 2^-60 .. 5e-324 and of 2^900, modes
that do not live, the seam of nk_fl_decay at tc / tau = 1/8, w_min and max_segments at their ends, launch shapes that leave lanes
idle, columns that die in different orders, start points on the planes of a map's grid -- and the inputs the host refuses.

What is compared how (the three rules of test_gpu_free_path.assert_rays):
  * the discrete outputs -- start points, end codes, segment counts, the counts of rays, casts, missed and capped -- are equal;
  * a ray's displacement relative to its own |D| and its flight time relative to itself, within <= 10 x the largest deviation
    measured on an MI355X for that case (profiles/free_path_margins.txt, "free-path edges"), never above test_gpu_free_path's 5e-14;
    where the measurement is 0 the test asks for the bits;
  * a mode's row equals wave_sum of the engine's own rays as bytes.
Every case is run three ways -- Engine.free_paths, column 0 of a one-column Engine.free_path_columns, Engine.free_path_map -- and the
three are compared as bytes, rows and per-ray outputs alike.  Every case's rays keep their facet sequence between fused and unfused
hit points on the CPU (test_free_path_edges_host.py), so no ray is left out of a comparison.  No non-finite coordinate and no
non-finite positive lifetime reaches a kernel here: those are refused on the host and tested as refusals; the NaN lifetime of 'dead'
takes no cast."""
import numpy as np
import pytest

import free_path_cases as FC
import free_path_edge_cases as E
from util import allclose, rel_err
from test_free_map_host import case_weights
from test_gpu_free_path import fp_engine, wave_sum, TOL_RAY_D, TOL_RAY_T, TOL_MODE_W
from test_gpu_free_sweep import assert_column_is_single
from test_gpu_free_map import assert_cells_are_the_rule, MODE_KEYS, RAY_KEYS

pytestmark = pytest.mark.gpu

# Per case, <= 10 x the deviation measured on an MI355X (profiles/free_path_margins.txt, "free-path edges"); 0: the kernel gave the
# restatement's bits and the test asks for them.  D: max |D_gpu - D_cpu| / |D_cpu|_2 of a ray, T: relative.
TOL_D = {'cell_planes': 1.1e-15, 'dead_ttp': 2.2e-15, 'dead_wire72': 1.1e-15, 'huge_tau_ttp': 7.7e-15, 'huge_tau_wire72': 0.0,
         'misses_ttp': 2.2e-15, 'misses_wire72': 3.3e-15, 'n1_ttp': 3.3e-15, 'n1_wire72': 2.2e-15, 'n63_ttp': 1.4e-14, 'n63_wire72': 3.3e-15,
         'n65_ttp': 1.4e-14, 'n65_wire72': 3.3e-15, 'one_segment': 3.3e-15, 'seam': 3.3e-15, 'tiny_tau': 0.0, 'wmin_one': 3.3e-15,
         'wmin_smallest': 1.7e-14,
         'columns_ttp_tiny_tau': 0.0, 'columns_ttp_dead': 0.0, 'columns_ttp_huge_tau': 2.2e-15, 'columns_ttp_plain': 2.2e-15,
         'columns_wire72_tiny_tau': 0.0, 'columns_wire72_dead': 0.0, 'columns_wire72_huge_tau': 0.0, 'columns_wire72_plain': 3.3e-15}
TOL_T = {'cell_planes': 2.9e-15, 'dead_ttp': 2.6e-15, 'dead_wire72': 1.7e-15, 'huge_tau_ttp': 0.0, 'huge_tau_wire72': 0.0,
         'misses_ttp': 2.6e-15, 'misses_wire72': 4.0e-15, 'n1_ttp': 2.5e-15, 'n1_wire72': 1.3e-15, 'n63_ttp': 1.7e-14, 'n63_wire72': 4.0e-15,
         'n65_ttp': 1.7e-14, 'n65_wire72': 5.1e-15, 'one_segment': 4.0e-15, 'seam': 3.3e-15, 'tiny_tau': 0.0, 'wmin_one': 4.0e-15,
         'wmin_smallest': 1.9e-14,
         'columns_ttp_tiny_tau': 0.0, 'columns_ttp_dead': 0.0, 'columns_ttp_huge_tau': 0.0, 'columns_ttp_plain': 2.6e-15,
         'columns_wire72_tiny_tau': 0.0, 'columns_wire72_dead': 0.0, 'columns_wire72_huge_tau': 0.0, 'columns_wire72_plain': 4.0e-15}
assert set(E.CASES) <= set(TOL_D) and set(TOL_D) == set(TOL_T)
assert max(TOL_D.values()) <= TOL_RAY_D == 5e-14 and max(TOL_T.values()) <= TOL_RAY_T == 5e-14
_ENG = {}


def engine(base):
    """One engine per set of tables for the whole module (the parity engines without particles)."""
    if base not in _ENG:
        _ENG[base] = fp_engine(FC.case(base), seed=99)
    return _ENG[base]


def three_ways(name):
    """The case through free_paths, as a one-column free_path_columns call and through free_path_map, each once (cached)."""
    def make():
        inp = E.inputs(name)
        eng, kw = engine(inp['base']), dict(E.call_args(inp), rays=True)
        w = case_weights(inp['ct'], inp['modes'])[1]
        lo, h, n = E.map_grid(inp)
        return dict(plain=eng.free_paths(inp['tau'], **kw), cols=eng.free_path_columns(inp['tau'][None, :], **kw),
                    map=eng.free_path_map(inp['tau'], w, lo, h, n, **kw), weight=w, grid=(lo, h, n))
    return FC.cached(('fp_edge_gpu', name), make)


def compare(name, got, ref, tol=None):
    """A call against the restatement of the same inputs: the module docstring's three rules, every ray."""
    tol = tol or name
    n = int(ref['n'])
    assert np.array_equal(got['ray_x0'], ref['ray_x0'])
    assert np.array_equal(got['ray_end'], ref['ray_end']), 'end codes differ'
    assert np.array_equal(got['ray_segments'], ref['ray_segments']), 'segment counts differ'
    big = np.abs(ref['ray_D']).max(axis=2)[..., None]                  # |D|_2 without squaring 2^900 v (a miss of the 'huge_tau' column)
    big = np.where(big > 0, big, 1.0)
    with np.errstate(over='ignore', under='ignore'):
        nrm = big * np.linalg.norm(ref['ray_D'] / big, axis=2)[..., None]
        nrm = np.where(nrm > 0, nrm, 1.0)
        ok_D = allclose(got['ray_D'] / nrm, ref['ray_D'] / nrm, rtol=0, atol=TOL_D[tol], tag=tol + ' D')
        worst_T = rel_err(got['ray_T'], ref['ray_T'], tag=tol + ' T', bound=TOL_T[tol])
    print('%s: %d rays, ends %s' % (tol, got['ray_end'].size, np.bincount(got['ray_end'].ravel(), minlength=5).tolist()))
    assert ok_D, 'displacements differ'
    assert worst_T <= TOL_T[tol], 'flight times differ'
    if TOL_D[tol] == 0.0:
        assert got['ray_D'].tobytes() == ref['ray_D'].tobytes()
    if TOL_T[tol] == 0.0:
        assert got['ray_T'].tobytes() == ref['ray_T'].tobytes()
    assert got['D'].tobytes() == wave_sum(got['ray_D']).tobytes() and got['T'].tobytes() == wave_sum(got['ray_T']).tobytes()
    with np.errstate(over='ignore', under='ignore'):
        assert rel_err(got['D2'], wave_sum(got['ray_D'] ** 2), tag=tol + ' D2', bound=n * 2.0 ** -53) <= n * 2.0 ** -53
    for k in ('p_res', 'p_wall', 'w_left', 'p_int'):
        assert allclose(got[k] / n, ref[k] / n, rtol=0, atol=TOL_MODE_W, tag=tol + ' ' + k), k
    assert allclose(got['hits'] / n, ref['hits'] / n, rtol=TOL_T[tol], atol=TOL_MODE_W, tag=tol + ' hits')
    assert np.isfinite(got['ray_D']).all() and np.isfinite(got['ray_T']).all()
    for k in FC.MODE_KEYS:                                              # (D2 of a miss with tau = 2^900 is inf on both sides)
        assert np.array_equal(np.isfinite(got[k]), np.isfinite(ref[k])), k


def assert_same_bytes(a, b, label):
    for k in MODE_KEYS + RAY_KEYS:
        assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), '%s differ in %s' % (label, k)
    for k in ('rays', 'casts', 'missed', 'capped', 'geometry_mode'):
        assert a['report'][k] == b['report'][k], (label, k)


@pytest.mark.parametrize('name', sorted(E.CASES))
def test_case_against_restatement(name):
    got, ref = three_ways(name)['plain'], E.run(name)
    for k in ('rays', 'casts', 'missed', 'capped'):
        assert got['report'][k] == ref['report'][k], k
    assert got['report']['geometry_mode'] == (2 if E.inputs(name)['base'] == 'wire72' else 1)
    compare(name, got, ref)


@pytest.mark.parametrize('name', sorted(E.CASES))
def test_three_ways(name):
    """free_paths, column 0 of a one-column call and the map call give the same bytes; the map's cells are free_map.tally of its own
    rays, its cell indices field.cell_index's."""
    inp, t = E.inputs(name), three_ways(name)
    assert_column_is_single(t['cols'], 0, t['plain'], name)
    assert t['cols']['report']['casts_shared'] == t['plain']['report']['casts']
    assert_same_bytes(t['map'], t['plain'], name + ': map and plain call')
    assert t['map']['report']['overflow'] == 0
    assert_cells_are_the_rule(t['map'], t['weight'], t['grid'], inp['ct'], inp['tau'], carries_weight=name != 'tiny_tau')


@pytest.mark.parametrize('name', E.MISSES)
def test_misses_bit_for_bit(name):
    inp, got = E.inputs(name), three_ways(name)['plain']
    out = inp['outside']
    v, tau = FC.group_vel(inp['ct'])[inp['modes']], inp['tau'][inp['modes']]
    assert (got['ray_end'][:, out] == 3).all() and (got['ray_segments'][:, out] == 1).all() and not (got['ray_end'][:, ~out] == 3).any()
    assert np.array_equal(got['ray_D'][:, out], np.broadcast_to((tau[:, None] * v)[:, None, :], (6, 32, 3)))        # one rounding per component
    assert np.array_equal(got['ray_T'][:, out], np.broadcast_to(tau[:, None], (6, 32)))
    assert got['report']['missed'] == 6 * 32
    # the missing rays alone, half a wave per mode: each one's share of p_int is 1, and it leaves nothing else
    only = engine(inp['base']).free_paths(inp['tau'], **dict(E.call_args(inp), n=32, x0=np.ascontiguousarray(inp['x0'][:, out]), rays=True))
    assert np.array_equal(only['p_int'], [32.0] * 6) and only['report']['missed'] == only['report']['rays'] == only['report']['casts'] == 192
    for k in ('hits', 'p_res', 'p_wall', 'w_left'):
        assert not only[k].any(), k
    assert only['ray_D'].tobytes() == np.ascontiguousarray(got['ray_D'][:, out]).tobytes() and only['D'].tobytes() == wave_sum(only['ray_D']).tobytes()
    # the map on the missing rays alone: the kernel's own cells take N, the K words and T, and nothing in words 10 to 12
    t = three_ways(name)
    lo, h, n = t['grid']
    m = engine(inp['base']).free_path_map(inp['tau'], t['weight'], lo, h, n, **dict(E.call_args(inp), n=32, x0=np.ascontiguousarray(inp['x0'][:, out]), rays=True))
    cells = m['cells']
    assert (m['ray_end'] == 3).all() and not m['ray_w'].any() and m['report']['overflow'] == 0
    assert cells[..., 0].sum() == 192 and cells[..., 1:10].any() and not cells[..., 10:13].any() and cells[..., 13].any()
    assert m['report']['clamped'] == 192                                 # they start outside the grid, which spans the bounds
    assert_cells_are_the_rule(m, t['weight'], t['grid'], inp['ct'], inp['tau'])
    assert not t['map']['ray_w'][t['map']['ray_end'] == 3].any()


def test_tiny_tau_bit_for_bit():
    inp, got = E.inputs('tiny_tau'), three_ways('tiny_tau')['plain']
    v, tau = FC.group_vel(inp['ct'])[inp['modes']], inp['tau'][inp['modes']]
    assert np.array_equal(got['ray_D'], np.broadcast_to((tau[:, None] * v)[:, None, :], (8, 64, 3)))
    assert np.array_equal(got['ray_T'], np.broadcast_to(tau[:, None], (8, 64)))
    assert (got['ray_segments'] == 1).all() and not got['ray_end'][inp['along']].any()
    assert np.array_equal(got['p_int'], [64.0] * 8)
    for k in ('hits', 'p_res', 'p_wall', 'w_left'):
        assert not got[k].any() and not np.signbit(got[k]).any(), k
    for k in FC.MODE_KEYS + ('ray_D', 'ray_T'):
        assert np.isfinite(got[k]).all(), k


@pytest.mark.parametrize('name', ['huge_tau_ttp', 'huge_tau_wire72'])
def test_huge_tau_is_ballistic(name):
    inp, got = E.inputs(name), three_ways(name)['plain']
    tc, fc = E.first_cast(inp['ct'], inp['modes'], inp['x0'])
    one = got['ray_segments'] == 1
    flown = tc[..., None] * FC.group_vel(inp['ct'])[inp['modes']][:, None, :]
    assert one.any() and np.isfinite(got['ray_D']).all() and np.isfinite(got['ray_T']).all()
    # wt = (2^900) (tc / 2^900) = tc exactly and D = one rounding of tc v: measured 0 against the oracle's tc on both geometries
    # (profiles/free_path_margins.txt), so the bits are asked for
    assert np.array_equal(got['ray_D'][one], flown[one]) and np.array_equal(got['ray_T'][one], tc[one])
    assert np.array_equal(got['hits'], got['ray_segments'].sum(axis=1))             # W = 1 at every hit, exactly


@pytest.mark.parametrize('name', ['dead_ttp', 'dead_wire72'])
def test_dead_exactly(name):
    inp, got = E.inputs(name), three_ways(name)['plain']
    d = inp['dead']
    assert not got['ray_end'][d].any() and not got['ray_segments'][d].any() and not got['ray_T'][d].any() and not got['ray_D'][d].any()
    assert np.array_equal(got['p_int'][d], [64.0] * 3) and np.array_equal(got['T'][d], [0.0] * 3) and not np.isnan(got['T']).any()
    assert got['report']['casts'] == got['ray_segments'][~d].sum()


def test_limits():
    one, small, seg = (three_ways(k) for k in ('wmin_one', 'wmin_smallest', 'one_segment'))
    # w_min = 1: every ray that goes on ends after its first segment with code 0, and w_left takes what is left of it, e
    inp, p, m = E.inputs('wmin_one'), one['plain'], one['map']
    assert (p['ray_segments'] == 1).all() and set(np.unique(p['ray_end'])) == {0, 1}
    tc, fc = E.first_cast(inp['ct'], inp['modes'], inp['x0'])
    e = np.exp(-tc / inp['tau'][inp['modes']][:, None])
    left = p['ray_end'] == 0
    assert p['w_left'].tobytes() == wave_sum(np.where(left, m['ray_w'], 0.0)).tobytes() and (m['ray_w'][left] > 0).all()
    assert rel_err(m['ray_w'][left], e[left], tag='w_min = 1: w_left', bound=2.2e-15) <= 2.2e-15          # (measured 2.2e-16: nk_exp_small against exp)
    # w_min = 5e-324: no ray is cut; reservoir or cap
    assert set(np.unique(small['plain']['ray_end'])) == {1, 4} and small['plain']['report']['capped'] == 192 and (small['plain']['ray_end'][:3] == 4).all()
    # max_segments = 1
    assert (seg['plain']['ray_segments'] == 1).all() and set(np.unique(seg['plain']['ray_end'])) == {1, 4}
    assert seg['plain']['w_left'].tobytes() == wave_sum(np.where(seg['plain']['ray_end'] == 4, seg['map']['ray_w'], 0.0)).tobytes()


@pytest.mark.parametrize('base', ['ttp', 'wire72'])
def test_columns(base):
    """One call whose columns are the lifetimes of 'tiny_tau', 'dead', 'huge_tau' and the plain table, on the 'misses' start points:
    every column is its single call as bytes and its restatement within the bounds; a miss ends all live columns at once, a column
    that is dead at the start takes no cast."""
    inp = E.inputs('misses_' + base)
    taus = E.column_taus(base)
    eng, kw = engine(base), dict(E.call_args(inp), rays=True)
    cols = eng.free_path_columns(taus, **kw)
    assert cols['columns'] == 4 and cols['report']['launches'] == 1
    out = inp['outside']
    for c, label in enumerate(E.COLUMN_NAMES):
        single = eng.free_paths(taus[c], **kw)
        assert_column_is_single(cols, c, single, 'columns ' + label)
        ref = E.run_column(base, c)
        for k in ('casts', 'missed', 'capped'):
            assert int(cols[k][c]) == ref['report'][k], (label, k)
        compare('columns %s %s' % (base, label), single, ref, tol='columns_%s_%s' % (base, label))
    seg, end = cols['ray_segments'], cols['ray_end']
    assert not seg[1].any() and not end[1].any() and cols['casts'][1] == 0 and np.array_equal(cols['p_int'][1], [64.0] * 6)
    for c in (0, 2, 3):
        assert (end[c][:, out] == 3).all() and (seg[c][:, out] == 1).all() and cols['missed'][c] == 192
    assert (seg[0] == 1).all() and (seg[0] <= seg[3]).all() and (seg[3] <= seg[2]).all()
    assert cols['report']['casts_shared'] == int(seg.max(axis=0).sum())


def test_cell_planes():
    from nanokappa_amd import field as FD
    inp, t = E.inputs('cell_planes'), three_ways('cell_planes')
    m = t['map']
    lo, h, n = t['grid']
    c, clamped = FD.cell_index(inp['x0'].reshape(-1, 3), lo, h, n)
    assert np.array_equal(m['ray_cell'].ravel(), (c[:, 0] * n[1] + c[:, 1]) * n[2] + c[:, 2])
    assert m['report']['clamped'] == int(clamped.sum()) == 2 * (96 - 8 * 3 * 2)
    hi = E.bounds(inp['ct'])[1]
    x = inp['x0'].reshape(-1, 3)
    cell = np.stack(np.unravel_index(m['ray_cell'].ravel(), n), axis=1)
    for a in range(3):                                                  # the upper boundary lands in the last cell
        assert (cell[x[:, a] == hi[a], a] == n[a] - 1).all() and (x[:, a] == hi[a]).any()
    assert m['report']['missed'] == 108 and not m['ray_w'][m['ray_end'] == 3].any()


# ------------------------------------------------------------------------------------------- what the host refuses
def entry_points(eng, inp):
    """name -> (call(tau, x0), refuse(tau, x0)) of the entry point on a case's inputs, with tau [M]; the column call takes two columns
    (the plain table and tau).  call goes through the binding and returns its result; refuse calls the C entry point itself with a
    report filled with ones beforehand and returns (rc, the error text, the report's bytes)."""
    import ctypes as C
    from nanokappa_amd import engine as EN
    kw = dict(E.call_args(inp), rays=True)
    w = case_weights(inp['ct'], inp['modes'])[1]
    lo, h, n = E.map_grid(inp)
    two = lambda tau: np.stack([inp['tau'], tau])

    def direct(fn, rep_type, tau, x0, columns=False, grid=False):
        a, pm, pr, out, ml = eng._free_path_call(fn, tau, kw['n'], kw['modes'], kw['max_segments'], kw['w_min'], x0, kw['seed'], False, columns=columns)
        rep = rep_type()
        C.memset(C.byref(rep), 0xff, C.sizeof(rep))
        args = [eng.h, C.byref(a)]
        keep = None
        if columns:
            args.append(2)
        if grid:
            g = EN.nk_free_path_grid()
            g.n[:], g.lo[:], g.h[:], g.weight = list(n), list(lo), list(h), EN._p(w)
            keep = np.zeros(tuple(n) + (16,), dtype=np.int64)
            args += [C.byref(g), keep.ctypes.data_as(C.POINTER(C.c_int64))]
        rc = getattr(eng.L, fn)(*(args + [C.byref(pm), None, C.byref(rep)]))
        assert not any(np.asarray(v).any() for v in out.values()) and (keep is None or not keep.any())         # nothing was written
        return rc, eng.L.nk_last_error(eng.h).decode(), bytes(rep)

    return {
        'nk_free_paths': (lambda tau, x0: eng.free_paths(tau, **dict(kw, x0=x0)),
                          lambda tau, x0: direct('nk_free_paths', EN.nk_free_path_report, tau, x0)),
        'nk_free_paths_columns': (lambda tau, x0: eng.free_path_columns(two(tau), **dict(kw, x0=x0)),
                                  lambda tau, x0: direct('nk_free_paths_columns', EN.nk_free_path_columns_report, two(tau), x0, columns=True)),
        'nk_free_paths_map': (lambda tau, x0: eng.free_path_map(tau, w, lo, h, n, **dict(kw, x0=x0)),
                              lambda tau, x0: direct('nk_free_paths_map', EN.nk_free_path_map_report, tau, x0, grid=True)),
    }


@pytest.mark.parametrize('base', ['ttp', 'wire72'])
def test_refusals(base):
    """A positive lifetime that is not finite, in any entry of tau (listed or not, any column), and a start point that is not finite
    are refused on all three entry points: NK_ERR_ARG from the C entry point, a text that names the entry, every byte of the returned
    report zero, no output written; through the binding an NkError.  Nothing ran -- the next ordinary call is the entry point's next
    call by its own count -- and it gives the bytes it gave before."""
    from nanokappa_amd.engine import NkError, ERR_ARG
    inp = E.inputs('n65_' + base)
    eng = engine(base)
    M = inp['ct']['M']
    unlisted = int(np.setdiff1d(np.arange(M), inp['modes'])[-1])
    infos = {'nk_free_paths': eng.free_paths_info, 'nk_free_paths_map': eng.free_path_map_info}
    for who, (call, refuse) in entry_points(eng, inp).items():
        before = call(inp['tau'], inp['x0'])
        info = infos[who]() if who in infos else None
        for m in (int(inp['modes'][2]), unlisted):
            tau = inp['tau'].copy()
            tau[m] = np.inf
            text = '%s: tau of mode %d is not finite' % (who, m) + (' (column 1)' if who == 'nk_free_paths_columns' else '')
            rc, said, rep = refuse(tau, inp['x0'])
            assert rc == ERR_ARG == -2 and said == text and rep == bytes(len(rep)), (rc, said)
            with pytest.raises(NkError, match=r'\(-2\)') as e:
                call(tau, inp['x0'])
            assert text in str(e.value), str(e.value)
        for bad, (li, s, a) in ((np.nan, (0, 0, 0)), (np.inf, (3, 64, 2)), (-np.inf, (5, 17, 1))):
            x0 = inp['x0'].copy()
            x0[li, s, a] = bad
            text = '%s: x0 of list entry %d, sample %d is not finite' % (who, li, s)
            rc, said, rep = refuse(inp['tau'], x0)
            assert rc == ERR_ARG and said == text and rep == bytes(len(rep)), (rc, said)
            with pytest.raises(NkError, match=r'\(-2\)') as e:
                call(inp['tau'], x0)
            assert text in str(e.value), str(e.value)
        if info is not None:
            assert infos[who]() == info                                 # the last report stays
        after = call(inp['tau'], inp['x0'])
        assert after['report']['calls'] == before['report']['calls'] + 1            # ten refusals in between: none counted
        for k in MODE_KEYS + RAY_KEYS:
            assert np.asarray(after[k]).tobytes() == np.asarray(before[k]).tobytes(), (who, k)
        tau = inp['tau'].copy()
        tau[unlisted], tau[int(inp['modes'][0])] = -np.inf, np.nan      # not positive: such modes do not live, and are taken
        dead = call(tau, inp['x0'])
        assert dead['report']['calls'] == after['report']['calls'] + 1
