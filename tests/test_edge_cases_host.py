"""The edge inputs of edge_cases.py are what they claim to be -- checked on the CPU with the exact references and the oracle alone,
so that test_gpu_edges.py cannot pass for want of a tie, a near-tie, a skipped wall or a fallback:  generic rays have ONE
admissible wall, the tie family ties exactly (in double: every quotient and cross product is exact), edge-aimed rays have at
least two admissible walls, the oracle always stays inside the admissible set, the oracle's classifier leaves the exact rule
only inside the rounding band of its 3-D squared distances, and the non-convex meshes really send rays into both fallbacks of
nk_find_boundary."""
import ctypes as C
import os
import sys
from fractions import Fraction as Fr

import numpy as np
import pytest

import edge_cases as EC
from util import rel_err

sys.path.insert(0, os.path.join(os.path.dirname(__file__), '..', 'oracle'))
import nk_oracle as O  # noqa: E402

c_dp, c_ip = O.c_dp, O.c_ip


def P(a, t=c_dp):
    return a.ctypes.data_as(t)


def oracle_cast(g, x, v):
    mesh = O.make_mesh(g)
    x, v = np.ascontiguousarray(x, dtype=float), np.ascontiguousarray(v, dtype=float)
    n = x.shape[0]
    xc, tc, fc = np.zeros((n, 3)), np.zeros(n), np.zeros(n, dtype=np.int32)
    O.lib().nko_find_boundary(C.byref(mesh), C.c_int64(n), P(x), P(v), P(xc), P(tc), P(fc, c_ip))
    return tc, fc


def test_cuboid_maps_differ_from_the_cube():
    Wc, Wq = EC.box_walls(EC.box_mesh('cube')), EC.box_walls(EC.box_mesh('cuboid'))
    assert list(Wc['facet']) == [0, 1, 2, 3, 4, 5] and list(Wc['face0']) == [0, 2, 4, 6, 8, 10]
    assert sorted(Wq['facet']) == [0, 1, 2, 3, 4, 5] and not np.array_equal(Wq['facet'], Wc['facet'])
    assert not np.array_equal(np.argsort(Wq['face0']), np.argsort(Wc['face0']))
    assert len({float(h) for h in Wq['hi']}) == 3
    # the oracle's own detection reads the same walls
    p = O.make_params()
    assert O.lib().nko_box_detect(C.byref(O.make_mesh(EC.box_mesh('cuboid'))), C.byref(p)) == 1
    assert [int(f) for f in p.box_facet] == [int(f) for f in Wq['facet']]


@pytest.mark.parametrize('name', ['cube', 'cuboid'])
def test_next_hit_families_are_what_they_claim(name):
    W = EC.box_walls(EC.box_mesh(name))
    fam = EC.box_next_families(name)
    for k in 'abc':
        ex = EC.exact_all(EC.exact_next_hit, W, *fam[k])
        assert all(len(e['adm']) == 1 and not e['tie'] and e['facet'] >= 0 for e in ex), k
    # (c): a quarter of tol in front of a wall skips it, four tol hit it
    x, v = fam['c']
    ex = EC.exact_all(EC.exact_next_hit, W, x, v)
    for i, e in enumerate(ex):
        a = int(np.argmin(np.minimum(np.abs(x[i] - W['lo']), np.abs(x[i] - W['hi']))))      # the axis of the wall close by
        near = 2 * a + (1 if v[i, a] > 0 else 0)
        d = abs(Fr(float(W['pos'][near])) - Fr(float(x[i, a]))) / abs(Fr(float(v[i, a])))
        if fam['c_ratio'][i] < 1:
            assert d < Fr(EC.TOL) / 2 and e['wall'] != near
        else:
            assert d > 2 * Fr(EC.TOL) and e['wall'] == near and e['value'] == d
    # (d): every ray ties exactly, and in double: the numerators, quotients and cross products are exact
    x, v = fam['d']
    ex = EC.exact_all(EC.exact_next_hit, W, x, v)
    assert len(ex) == 60 and all(e['tie'] for e in ex)
    assert sum(len(e['per_facet']) == 3 for e in ex) == 24
    for i, e in enumerate(ex):
        tied = [w for w in range(6) if e['per_facet'].get(int(W['facet'][w])) == e['value']]
        assert len(tied) >= 2 and e['wall'] == min(tied, key=lambda w: W['face0'][w])
        md = []
        for w in tied:
            a = w // 2
            m = (W['pos'][w] - x[i, a]) if w % 2 else (x[i, a] - W['pos'][w])
            assert Fr(float(m)) == abs(Fr(float(W['pos'][w])) - Fr(float(x[i, a]))) == 32
            assert Fr(float(m / abs(v[i, a]))) == e['value']
            md.append((m, abs(v[i, a])))
        for (m0, d0) in md:
            for (m1, d1) in md:
                assert Fr(float(m0 * d1)) == Fr(float(m0)) * Fr(float(d1)) == Fr(float(m1 * d0))
    # (e): at least two admissible walls on every ray
    ex = EC.exact_all(EC.exact_next_hit, W, *fam['e'])
    assert all(len(e['adm']) >= 2 for e in ex)
    assert sum(len(e['adm']) == 3 for e in ex) >= 200
    # (f): the misses miss, the rays along one axis hit the far wall
    x, v = fam['f']
    ex = EC.exact_all(EC.exact_next_hit, W, x, v)
    nm = fam['f_nmiss']
    assert all(e['facet'] == -1 for e in ex[:nm])
    for i in range(nm, x.shape[0]):
        a = int(np.argmax(np.abs(v[i])))
        assert ex[i]['wall'] == 2 * a + (1 if v[i, a] > 0 else 0) and ex[i]['value'] == Fr(float(W['hi'][a] - W['lo'][a])) / Fr(37.5)


@pytest.mark.parametrize('name', ['cube', 'cuboid'])
def test_first_hit_families_are_what_they_claim(name):
    W = EC.box_walls(EC.box_mesh(name))
    fam = EC.box_first_families(name)
    for k, nw in (('beyond1', 1), ('beyond2', 2), ('beyond3', 3), ('next', 1), ('mixed', 1)):
        ex = EC.exact_all(EC.exact_first_hit, W, *fam[k])
        assert all(len(e['per_facet']) == nw and len(e['adm']) == 1 and not e['tie'] for e in ex), k
    for k in ('on', 'away'):
        assert all(e['facet'] == -1 for e in EC.exact_all(EC.exact_first_hit, W, *fam[k])), k
    ex = EC.exact_all(EC.exact_first_hit, W, *fam['ties'])
    assert len(ex) == 40 and all(e['tie'] and len(e['adm']) == len(e['per_facet']) for e in ex)
    x, v = fam['ties']
    for i, e in enumerate(ex):
        assert e['value'] == Fr(1, 8) / (Fr(1, 4) if i < 20 else 16)          # speeds 2^-2, then 2^4


@pytest.mark.parametrize('name', ['cube', 'cuboid'])
def test_oracle_stays_in_the_admissible_set(name):
    """The oracle picks by rounded quotients: on near-ties it may name another wall than the cross products would, never one
    outside the admissible set; on exact ties the lowest face index."""
    g = EC.box_mesh(name)
    W = EC.box_walls(g)
    fam = EC.box_next_families(name)
    differs = 0
    for k in 'abcdef':
        x, v = fam[k]
        ex = EC.exact_all(EC.exact_next_hit, W, x, v)
        tc, fc = oracle_cast(g, x, v)
        if k == 'c':
            # a quarter of tol in front of a wall: the ray leaves through that wall, which is skipped, and meets every other
            # wall's plane outside its rectangle -- the all-faces search misses, where the box rule (no face test: its particles
            # are inside) names the next wall.  Only the rays at four tol are compared with the oracle.
            skip = fam['c_ratio'] < 1
            assert np.all(fc[skip] == -1) and np.all(np.isinf(tc[skip]))
            x, v, tc, fc, ex = x[~skip], v[~skip], tc[~skip], fc[~skip], [e for e, s_ in zip(ex, skip) if not s_]
        assert all(int(fc[i]) in ex[i]['adm'] for i in range(x.shape[0])), k
        if k != 'e':
            assert np.array_equal(fc, [e['facet'] for e in ex]), k
        else:
            differs = sum(int(fc[i]) != e['facet'] for i, e in enumerate(ex))
        hit = fc >= 0
        assert np.all(np.isinf(tc[~hit]))
        te = np.array([float(ex[i]['per_facet'][int(fc[i])]) for i in np.nonzero(hit)[0]])
        assert rel_err(tc[hit], te) < 1e-12, k
    print('%s: oracle names another wall than the exact minimum on %d of %d edge-aimed rays' % (name, differs, fam['e'][0].shape[0]))


def oracle_classify(d, x, interp=1):
    S = d['centers'].shape[0]
    sv = O.make_subvols(d['centers'], np.ones(S), 0, d['axis'], interp)
    x = np.ascontiguousarray(x)
    out = np.zeros(x.shape[0], dtype=np.int32)
    O.lib().nko_classify(C.byref(sv), C.c_int64(x.shape[0]), P(x), P(out, c_ip))
    return out


def test_classifier_oracle_leaves_the_exact_rule_only_inside_its_rounding_band():
    n_far = n_far_out = n_diff = 0
    for name, d in sorted(EC.slice_sets().items()):
        x, off = EC.slice_points(name)
        idx, small = EC.slice_reference(name)
        got = oracle_classify(d, x)
        assert np.abs(got - idx).max() <= 1, name
        assert np.array_equal(got[~small], idx[~small]), name
        n_diff += int((got != idx).sum())
        far = np.isfinite(off) & (off >= 1e-12)
        n_far += int(far.sum())
        n_far_out += int((far & ~small).sum())
    print('oracle differs from the exact nearest centre on %d points; %d of %d offsets >= 1e-12 A lie outside the band' % (n_diff, n_far_out, n_far))
    assert n_diff > 0
    assert n_far_out >= 0.8 * n_far


@pytest.mark.parametrize('name', ['box200ttp', 'cyl', 'corrugated', 'castle'])
def test_lds_mesh_families_and_fallbacks(name):
    """The NumPy all-faces reference equals the oracle bit for bit, so its per-plane bookkeeping describes what the engine's
    search meets: on the non-convex meshes at least 200 rays whose nearest admissible plane has no passing face and at least 100
    with two planes tied for the smallest t."""
    g = EC.lds_mesh(name)
    assert np.asarray(g['face_normals']).shape[0] <= 256
    L = EC.lds_families(name)
    ref = L['ref']
    tc, fc = oracle_cast(g, L['x'], L['v'])
    assert np.array_equal(fc, ref['fc']) and np.array_equal(tc, ref['tc'])
    assert all(int(fc[i]) in ref['adm'][i] for i in range(fc.shape[0]))
    fam = L['fam']
    for k in ('generic', 'surface', 'outside', 'axis', 'edge', 'vertex'):
        assert fam[k].shape[0] >= 100, k
    assert ref['hit'][fam['generic']].all() and ref['hit'][fam['surface']].sum() >= 100
    out = ref['hit'][fam['outside']]
    assert out.sum() >= 50 and (~out).sum() >= 50
    if name != 'corrugated':                      # (its flanks are single triangles between rings of different radii)
        assert fam['diagonal'].shape[0] >= 50
    multi = np.array([len(a) for a in ref['adm']]) > 1
    for k in ('diagonal', 'edge', 'vertex'):      # aimed well enough that two faces pass at the same t (to 1e-12)
        if k in fam:
            assert ref['close2'][fam[k]].mean() >= 0.8, (k, ref['close2'][fam[k]].mean())
    print('%s: %d rays, %d nearest-plane-without-face, %d plane ties, %d near-tied facets' % (name, fc.shape[0], ref['noface'].sum(), ref['planetie'].sum(), multi.sum()))
    if name in EC.NONCONVEX_ARGS:
        assert ref['noface'].sum() >= 200
        assert ref['planetie'].sum() >= 100


def test_tau_windows_of_the_settings_differ():
    from util import golden_phonon
    g = np.asarray(golden_phonon().tables()['T_grid'], dtype=float)
    rows = {k: EC.tau_window(g, *v)[0] for k, v in EC.TAU_SETTINGS.items()}
    assert rows == dict(all300=9, lowest=0, highest=18, wide=9, node=11)
    assert EC.tau_window(g[10:12], 300.0, 300.0) is None and EC.tau_window(g[9:12], 300.0, 300.0)[0] == 0
