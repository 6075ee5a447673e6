"""The device lookups at their edges, through the taps: the box-wall functions on tied, nearly tied, wall-hugging and missing
rays; nk_find_boundary over the LDS planes on rays through edges, vertices and quad diagonals and into both of its fallbacks;
nk_classify / nk_interp_T on and next to slice edges, centres, grid bisectors and outside the box; nk_lifetime on the nodes and
window borders of its table; the energy tables on their nodes and beyond their ends.

Engine and oracle legitimately differ at some of these inputs (rounded quotients against cross products, rounded 3-D distances
against a 1-D comparison), so the references are exact (edge_cases.py, fractions.Fraction on the doubles); the oracle is
compared where test_edge_cases_host.py shows that it is decided.  Needs a real MI355X: run with `pytest -m gpu`."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import edge_cases as EC
from util import golden_phonon, rel_err, allclose, ulp_err, TOL_NTS

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'oracle'))


def mesh_engine(g, dt=1.0):
    """An engine with the material, the mesh and one subvolume: all the ray taps need."""
    from nanokappa_amd.engine import Engine
    eng = Engine(0, 1)
    eng.set_material(golden_phonon().tables())
    eng.set_mesh(g)
    b = np.asarray(g['bounds'], dtype=float)
    eng.set_subvolumes(0.5 * (b[0] + b[1])[None, :], np.ones(1), 0, 0, 1, np.full(1, 300.0))
    eng.set_params(dt=dt)
    assert float(g.get('tol', EC.TOL)) == EC.TOL
    return eng


def exact_t(ex, facets):
    """The exact t of the wall named `facets[i]` on ray i, as doubles (nan where that wall has none)."""
    return np.array([EC.hi_lo(e['per_facet'].get(int(f)))[0] for e, f in zip(ex, facets)])


@pytest.mark.parametrize('name', ['cube', 'cuboid'])
def test_box_next_hit(name):
    """nk_box_next_hit (which = 2) against the exact cast: the facet is the exact one where one wall is admissible, the lowest
    face index on exact ties, some admissible wall on near-ties (edge-aimed rays), -1 with t = inf on misses; t within 1e-12
    of the exact t of the wall named; and on every family but the near-ties bit-equal to the general search over the LDS planes
    (nk_device.h: "the very quotient the general search returns").  A quarter of tol in front of a wall the box rule skips that
    wall and names the next one, where the general search misses (the ray has left the box when it meets the next plane)."""
    g = EC.box_mesh(name)
    W = EC.box_walls(g)
    fam = EC.box_next_families(name)
    eng = mesh_engine(g)
    for k in 'abcdef':
        x, v = fam[k]
        ex = EC.exact_all(EC.exact_next_hit, W, x, v)
        want = np.array([e['facet'] for e in ex])
        t, f = eng.box_hit(2, x, v)
        assert all(int(f[i]) in ex[i]['adm'] for i in range(x.shape[0])), k
        if k != 'e':
            assert np.array_equal(f, want), k
        hit = want >= 0
        assert np.array_equal(f >= 0, hit) and np.all(np.isinf(t[~hit])) and np.all(t[~hit] > 0), k
        assert rel_err(t[hit], exact_t(ex, f)[hit], tag=k, bound=1e-12) < 1e-12, k
        if k != 'e':
            xc, tc, fc = eng.find_boundary(x, v)
            same = np.ones(x.shape[0], dtype=bool) if k != 'c' else fam['c_ratio'] > 1
            assert np.array_equal(fc[same], f[same]), k
            assert rel_err(t[same], tc[same], tag=k + ' bit-equal', bound=0) == 0.0 and np.array_equal(t[same], tc[same]), k
            assert np.all(fc[~same] == -1) and np.all(np.isinf(tc[~same])), k
    # (c) once more in words: tol / 4 skips the wall in front, 4 tol returns it at t = 4 tol
    x, v = fam['c']
    t, f = eng.box_hit(2, x, v)
    near = fam['c_ratio'] > 1
    assert rel_err(t[near], np.full(near.sum(), 4.0 * EC.TOL), bound=1e-4) < 1e-4 and np.all(t[~near] > 1e-3)
    assert fam['f_nmiss'] == 6 and np.all(eng.box_hit(2, *fam['f'])[1][:6] == -1)
    eng.close()


@pytest.mark.parametrize('dt', [1.0, 2.0])
@pytest.mark.parametrize('name', ['cube', 'cuboid'])
def test_box_out_and_first_hit(name, dt):
    """nk_box_out (which = 0) equals the exact predicate "beyond a wall it flies towards" on every point: on a wall is not out
    (strict comparison), one nextafter beyond is, beyond a wall it flies away from is not.  nk_box_first_hit (which = 1) names
    the exact earliest-crossed wall (lowest face index on exact ties) and its time in timesteps.

    Bound on nts = -(nb * nk_rcp(db)) * inv_dt against the exact -(num / den) / dt, in units u = 2^-53 relative:
      nb = fl(x_a - wall)      one rounding of the exact num                      <= 1 u
      db = |v_a|               exact
      nk_rcp(db)               <= 1 ulp of 1 / db (tests/test_gpu_scalar_math.py)  <= 2 u
      nb * rcp                 one rounding                                       <= 1 u
      * inv_dt                 dt a power of two here: exact
    together <= 4 u (second-order terms ~u^2), and a relative error of e u is below e ulps of the result (spacing(r) > u |r|):
    4 ulps.  Underflow (a point one denormal beyond the wall at -0.0) stays within one spacing of zero."""
    g = EC.box_mesh(name)
    W = EC.box_walls(g)
    eng = mesh_engine(g, dt=dt)
    from fractions import Fraction as Fr
    for k, (x, v) in sorted(EC.box_first_families(name).items()):
        ex = EC.exact_all(EC.exact_first_hit, W, x, v)
        out = np.array([e['facet'] >= 0 for e in ex])
        o, fo = eng.box_hit(0, x, v)
        assert np.array_equal(o, out.astype(float)) and np.all(fo == -1), k
        nts, f = eng.box_hit(1, x, v)
        assert np.array_equal(f, [e['facet'] for e in ex]), k
        assert all(int(f[i]) in ex[i]['adm'] for i in range(x.shape[0])), k
        if out.any():
            q = [EC.hi_lo(-e['value'] / Fr(dt)) for e in ex if e['facet'] >= 0]
            hi, lo = np.array([a for a, _ in q]), np.array([b for _, b in q])
            assert allclose(nts[out], hi, rtol=0, atol=TOL_NTS, tag=k), k
            assert ulp_err(nts[out], hi, lo, tag=k, bound=4) <= 4.0, k
            assert np.all(nts[out] <= 0.0), k
    eng.close()


@pytest.mark.parametrize('name', ['box200ttp', 'cyl', 'corrugated', 'castle'])
def test_find_boundary_lds_edges(name):
    """nk_find_boundary over the LDS planes against the all-faces float64 reference (bit-equal to the oracle,
    test_edge_cases_host.py): generic rays, starts on the surface and outside, axis-parallel rays, rays through quad diagonals,
    edges and vertices, rays whose nearest admissible plane has no passing face and rays with two planes tied for the smallest t
    (both fallbacks of the search; counted on the host).  The facet lies in the admissible set and is the oracle's wherever that
    set has one element or faces tie exactly (then the lowest face index); t within 1e-12 of the oracle's; misses are inf."""
    g = EC.lds_mesh(name)
    assert np.asarray(g['face_normals']).shape[0] <= 256 and len(g['bound_cond']) <= 256      # NK_LDS_FACES: the tables sit in LDS
    L = EC.lds_families(name)
    ref = L['ref']
    eng = mesh_engine(g)
    xc, tc, fc = eng.find_boundary(L['x'], L['v'])
    n = fc.shape[0]
    assert all(int(fc[i]) in ref['adm'][i] for i in range(n))
    one = np.array([len(a) == 1 for a in ref['adm']])
    exact_tie = (ref['T'] == ref['tc'][:, None]).sum(axis=1) > 1
    decided = one | exact_tie | ~ref['hit']
    assert decided.mean() > 0.9 and exact_tie[ref['hit']].sum() > 0
    assert np.array_equal(fc[decided], ref['fc'][decided])
    if 'diagonal' in L['fam']:
        d = L['fam']['diagonal']
        assert np.array_equal(fc[d], ref['fc'][d])
    hit = ref['hit']
    assert np.array_equal(fc >= 0, hit) and np.all(np.isinf(tc[~hit]))
    assert rel_err(tc[hit], ref['tc'][hit], bound=1e-12) < 1e-12
    for k in ('noface', 'planetie'):
        m = ref[k]
        if m.any():
            assert np.array_equal(fc[m & decided], ref['fc'][m & decided]) and rel_err(tc[m & hit], ref['tc'][m & hit], tag=k, bound=1e-12) < 1e-12
    eng.close()


@pytest.fixture(scope='module')
def material_engine():
    from nanokappa_amd.engine import Engine
    eng = Engine(0, 1)
    eng.set_material(golden_phonon().tables())
    yield eng
    eng.close()


def oracle_classify(centers, kind, axis, x):
    import nk_oracle as O
    S = centers.shape[0]
    sv = O.make_subvols(centers, np.ones(S), kind, axis, 1 if kind == 0 else 2)
    x = np.ascontiguousarray(x)
    out = np.zeros(x.shape[0], dtype=np.int32)
    O.lib().nko_classify(C.byref(sv), C.c_int64(x.shape[0]), x.ctypes.data_as(O.c_dp), out.ctypes.data_as(O.c_ip))
    return out


@pytest.mark.parametrize('name', sorted(EC.slice_sets()))
def test_slice_lookups_at_edges(name, material_engine):
    """nk_classify on slices equals the exact nearest centre on EVERY point (ties to the lower index, points outside the box
    to the end slices), and the oracle outside its rounding band.  nk_interp_T: 'nearest' (kind 0) and nearest-centre (kind 2)
    return T_sv[idx] of the bounds rule / the exact nearest centre bit for bit; 'linear' (kind 1) is within 2 ulps of the exact
    value of the oracle's formula slope (xa - c) + T with the left bracket on a centre (one rounding of xa - c, of the product
    unless fused, of the sum; the product is below a tenth of T here); one slice returns T_sv[0] everywhere."""
    eng = material_engine
    d = EC.slice_sets()[name]
    cen, a, Tsv = d['centers'], d['axis'], d['T_sv']
    S = cen.shape[0]
    x, _ = EC.slice_points(name)
    idx, small = EC.slice_reference(name)
    c = np.ascontiguousarray(cen[:, a])
    eng.set_subvolumes(cen, np.ones(S), 0, a, 1, Tsv)
    got = eng.classify(x)
    assert np.array_equal(got, idx)
    orc = oracle_classify(cen, 0, a, x)
    assert np.array_equal(got[~small], orc[~small])
    assert got[-8:-5].tolist() == [0, 0, 0] and got[-5:-2].tolist() == [S - 1] * 3          # outside either end
    T1 = eng.eval('interp_T', x)
    if S == 1:
        assert rel_err(T1, np.full(x.shape[0], Tsv[0]), tag='S=1', bound=0) == 0.0
    else:
        q, _ = EC.exact_linear_T(c, Tsv, x[:, a])
        hi, lo = (np.array(v) for v in zip(*[EC.hi_lo(r) for r in q]))
        assert ulp_err(T1, hi, lo, tag='linear', bound=2) <= 2.0
    for kind, want in ((0, EC.nearest_bounds_rule(c, x[:, a])), (2, idx)):
        eng.set_subvolumes(cen, np.ones(S), 0, a, kind, Tsv)
        T = eng.eval('interp_T', x)
        assert rel_err(T, Tsv[want], tag='kind %d' % kind, bound=0) == 0.0 and np.array_equal(T, Tsv[want]), kind


def test_grid_classify_at_bisectors(material_engine):
    """3-D nearest centre: points exactly on bisector planes, edges and corners of the cells go to the lowest index of the tied
    centres (all distances exact in double), the same points moved by a few ulps to one of them, random points to the oracle's."""
    eng = material_engine
    G = EC.grid_case()
    cen = G['centers']
    S = cen.shape[0]
    Tsv = 290.0 + np.arange(S, dtype=float)
    eng.set_subvolumes(cen, np.ones(S), 1, 0, 2, Tsv)
    tied = EC.exact_nearest_3d(cen, G['tie'])
    assert all(len(t) >= 2 for t in tied) and max(len(t) for t in tied) == 8
    got = eng.classify(G['tie'])
    assert np.array_equal(got, [t[0] for t in tied])
    assert np.array_equal(got, oracle_classify(cen, 1, 0, G['tie']))
    gm = eng.classify(G['moved'])
    assert all(int(s) in t for s, t in zip(gm, tied))
    assert np.array_equal(eng.classify(G['rand']), oracle_classify(cen, 1, 0, G['rand']))
    T = eng.eval('interp_T', G['tie'])
    assert rel_err(T, Tsv[got], bound=0) == 0.0


LIFETIME_ULPS = 4.0


def check_lifetime(eng, tb, lo, hi, seed, prev_row=-1):
    """One setting of the subvolume temperatures: returns the window's row.  prev_row: the row of the setting before it on this
    engine; where the window has to move, tau_rebuilds must rise."""
    g = np.asarray(tb['T_grid'], dtype=float)
    tau = np.asarray(tb['lifetime'], dtype=float).reshape(g.shape[0], -1)
    active = np.nonzero(np.all(tau > 0, axis=0))[0]
    ratio = tau[1:, active] / tau[:-1, active]
    assert max(ratio.max(), 1.0 / ratio.min()) <= 1.06                # what LIFETIME_ULPS assumes of the table
    S = 20
    before = eng.timing()['tau_rebuilds']
    eng.set_subvolumes(np.tile(np.linspace(5.0, 195.0, S)[:, None], (1, 3)), np.ones(S), 0, 0, 1, np.linspace(lo, hi, S))
    win = EC.tau_window(g, lo, hi)
    if prev_row != -1 and win is not None:
        assert win[0] != prev_row and eng.timing()['tau_rebuilds'] == before + 1
    T, bad = EC.lifetime_temperatures(g, win, seed)
    rng = np.random.default_rng(seed)
    mode = active[rng.integers(0, active.shape[0], T.shape[0])].astype(np.int32)
    got = eng.eval('lifetime', T, mode)
    hi_, lo_ = (np.array(v) for v in zip(*[EC.hi_lo(r) for r in EC.exact_lifetime(g, tau, T, mode)]))
    assert ulp_err(got, hi_, lo_, bound=LIFETIME_ULPS) <= LIFETIME_ULPS
    assert rel_err(got, hi_, bound=1e-12) < 1e-12
    assert np.all(np.isnan(eng.eval('lifetime', bad, mode[:bad.shape[0]])))
    # either side of every grid node (window borders among them: T == g0 reads the table, nextafter(g0) the packed rows) the
    # values differ by no more than the table's slope allows, plus the bound on each
    below, above = g[:-1], np.nextafter(g[:-1], np.inf)
    m = active[rng.integers(0, active.shape[0], below.shape[0])].astype(np.int32)
    slope = np.abs(np.diff(tau[:, m], axis=0)).max() / np.diff(g).min() / tau[:, m].min()
    bound = slope * np.spacing(g[-1]) + 2 * LIFETIME_ULPS * 2.0 ** -52
    assert rel_err(eng.eval('lifetime', above, m), eng.eval('lifetime', below, m), tag='across a node', bound=bound) <= bound
    return None if win is None else win[0]


def test_lifetime_windows_nodes_and_ends():
    """nk_lifetime against the exact linear interpolation of the table's doubles, on every grid node and window value +-1 ulp,
    midpoints and random T, for five settings of the subvolume temperatures that move the packed window (g0, g2] across the
    table (tau_rebuilds rises with each), and for tables of two and three rows (no window / the window is the table); NaN one
    ulp outside the table, at +-inf and NaN.

    Bound, in u = 2^-53 relative to the result r = t0 (1 - y) + t1 y, 0 <= y <= 1, t0, t1 > 0 within 6 % of each other:
      window form   y = fl(fl(T - g) * ig): T - g is exact (Sterbenz: g <= T <= 2 g), ig = fl(1 / 10) 1 u, the product 1 u: y (1 + 2u)
      division form y = fl(fl(T - g) / fl(g' - g)): both differences exact, the quotient 1 u
      1 - y         one rounding: (1 - y)(1 + u) - 2u y
      the two products and the sum, one rounding each unless fused
    r' - r <= 2u y |t1 - t0| + u (2 t0 (1 - y) + t1 y) + u r <= (0.12 + 2 + 1) u r < 3.2 u r (window), less for the division
    form; a relative error of e u is below e ulps: 4 ulps holds both, and is 9e-16, well inside 1e-12."""
    from nanokappa_amd.engine import Engine
    tb = golden_phonon().tables()
    eng = Engine(0, 1)
    eng.set_material(tb)
    rows = []
    for seed, k in enumerate(('all300', 'lowest', 'wide', 'highest', 'node')):       # consecutive settings never share a window
        rows.append(check_lifetime(eng, tb, *EC.TAU_SETTINGS[k], seed=seed, prev_row=rows[-1] if rows else -1))
    assert rows == [9, 0, 9, 18, 11]
    eng.close()
    for rws in ([10, 11], [9, 10, 11]):
        cut = EC.cut_tables(tb, rws)
        eng = Engine(0, 1)
        eng.set_material(cut)
        assert check_lifetime(eng, cut, 300.0, 300.0, seed=7) == (None if len(rws) == 2 else 0)
        eng.close()


def test_energy_tables_nodes_and_fill(material_engine):
    """nk_T_of_E / nk_E_of_T: on a node the table value bit for bit, outside the table the fill values, elsewhere within 2 ulps
    of the exact interpolation (the slope's two roundings and the product's act on the small increment over the node below)."""
    eng = material_engine
    tb = golden_phonon().tables()
    eng.set_subvolumes(np.array([[100.0, 100.0, 100.0]]), np.ones(1), 0, 0, 1, np.full(1, 300.0))
    Ta, Ea = np.asarray(tb['T_array'], dtype=float), np.asarray(tb['energy_array'], dtype=float)
    g = np.asarray(tb['T_grid'], dtype=float)
    for what, xs, ys, fill in (('T_of_E', Ea, Ta, (g.min(), g.max())), ('E_of_T', Ta, Ea, (Ea[0], Ea[-1]))):
        nodes, inner, outside = EC.table_points(xs, seed=len(what))
        got = eng.eval(what, nodes)
        assert rel_err(got, ys, tag=what + ' nodes', bound=0) == 0.0 and np.array_equal(got, ys)
        got = eng.eval(what, outside)
        assert rel_err(got, [fill[0], fill[0], fill[1], fill[1]], tag=what + ' fill', bound=0) == 0.0
        hi, lo = (np.array(v) for v in zip(*[EC.hi_lo(r) for r in EC.exact_interp(xs, ys, inner)]))
        assert ulp_err(eng.eval(what, inner), hi, lo, tag=what, bound=2) <= 2.0
