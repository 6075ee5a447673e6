"""The face-tree ray cast (nk_find_boundary_tree: nk_ray_f32, nk_ray_box, nk_walk_boxes, nk_tree_leaf, nk_tree_skip, and the
builder in nk_set_mesh) at its edges, through the taps Engine.find_boundary and Engine.tree_info.  Every part of the tree is a
filter in front of face arithmetic that is the reference's statement by statement; a wrong filter shows as a missed or
mis-attributed hit on a few rays, so the rays are aimed: lds_families' generator (edges, quad diagonals, vertices, exact ties,
starts on and outside the surface) on three tree-sized meshes, speeds over seven orders of magnitude, components that are zero,
denormal or below the float range of 1 / v, hits along the whole length of 60 000 A slivers, starts up to 1e6 A away (the |x| term
of the slab test's widening, and tmax at near-ties after long flights), rays inside and across the walls of
the tree's own boxes, and starts on a cap with the facet skip engaged.  test_tree_edges_host.py shows on the CPU that these
inputs are what they claim.  Needs a real MI355X: run with `pytest -m gpu`."""
import numpy as np
import pytest

import edge_cases as EC
from util import golden_phonon, rel_err

pytestmark = pytest.mark.gpu

MESHES = ['wire72', 'star', 'longwire']
FACES = {'wire72': 288, 'star': 576, 'longwire': 288}


def tree_engine(name):
    """An engine with the material, the mesh and one subvolume: all the ray taps need.  The tree is built here (nk_set_mesh reads
    NK_TREE_SPLIT and NK_NO_TREE)."""
    from nanokappa_amd.engine import Engine
    g = EC.tree_mesh(name)
    eng = Engine(0, 1)
    eng.set_material(golden_phonon().tables())
    eng.set_mesh(g)
    b = np.asarray(g['bounds'], dtype=float)
    eng.set_subvolumes(0.5 * (b[0] + b[1])[None, :], np.ones(1), 0, 0, 1, np.full(1, 300.0))
    eng.set_params(dt=1.0)
    assert float(g.get('tol', EC.TOL)) == EC.TOL
    return eng


def all_rays(name, eng=None):
    """tree_families plus `boxwall`, whose rays need the boxes of the device's tree: made once per process from the default tree
    (eng must then be given) and shared.  {x, v, fam, ref-like dict of fc, tc, hit, adm, decided, tie}."""
    def make():
        L = EC.tree_families(name)
        B = EC.boxwall_rays(EC.tree_mesh(name), eng.tree_info(boxes=True))
        n0 = L['x'].shape[0]
        fam = dict(L['fam'], boxwall=np.arange(n0, n0 + B['x'].shape[0]))
        d0, t0 = EC.decided(L['ref'])
        d1, t1 = EC.decided(B['ref'])
        cat = lambda k: np.concatenate([L['ref'][k], B['ref'][k]])
        return dict(x=np.concatenate([L['x'], B['x']]), v=np.concatenate([L['v'], B['v']]), fam=fam, fc=cat('fc'), tc=cat('tc'),
                    hit=cat('hit'), adm=L['ref']['adm'] + B['ref']['adm'], decided=np.concatenate([d0, d1]),
                    tie=np.concatenate([t0, t1]), nboxes=B['nboxes'])
    return EC.cached(('tree_all', name), make)


def shape_of(name, monkeypatch=None, split=None):
    def make():
        eng = tree_engine(name)
        info = eng.tree_info()
        eng.close()
        return info
    if split is None:
        return EC.cached(('tree_shape', name), make)
    monkeypatch.setenv('NK_TREE_SPLIT', str(split))
    out = make()
    monkeypatch.delenv('NK_TREE_SPLIT')
    return out


@pytest.mark.parametrize('name', MESHES)
def test_tree_shape(name, monkeypatch):
    """What nk_set_mesh built: a tree (NG = 1) of at least three levels under a top family of 2..4 nodes, every level a quarter of
    the one below (rounded up), the leaves' four slots holding the references and the padding between them; on longwire every
    60 000 A side triangle enters as several references, and as one with NK_TREE_SPLIT=0.  tree_info changes nothing: asked
    twice, with and without the boxes, it says the same."""
    eng = tree_engine(name)
    info = eng.tree_info()
    full = eng.tree_info(boxes=True)
    assert {k: v for k, v in full.items() if k not in ('family_boxes', 'leaf_boxes')} == info == eng.tree_info()
    eng.close()
    EC.cached(('tree_shape', name), lambda: info)
    F = FACES[name]
    assert info['NG'] == 1 and info['tree_top'] >= 2 and 2 <= info['top_family'] <= 4
    ln = info['level_nodes']
    assert len(ln) == info['tree_top'] + 1 and ln[0] == info['tree_leaves'] and ln[-1] == info['top_family']
    assert all(ln[l + 1] == (ln[l] + 3) // 4 for l in range(len(ln) - 1))
    assert info['references'] + info['pad_slots'] == 4 * info['tree_leaves'] and info['references'] >= F
    # the boxes as copied out: per level the nodes and the padding up to a multiple of four; real boxes are ordered and lie within
    # tree_bound (taken from the doubles; the floats are rounded outwards by less than two ulps, 2^-22 relative), padding boxes are
    # inverted; every leaf's slots hold 2 to 4 references
    assert [b.shape[0] for b in full['family_boxes']] == [(c + 3) // 4 * 4 for c in ln]
    for c, b in zip(ln, full['family_boxes']):
        assert np.all(b[:c, :3] <= b[:c, 3:]) and np.all(b[c:, :3] > b[c:, 3:])
        assert np.abs(b[:c].astype(np.float64)).max() <= info['tree_bound'] * (1.0 + 2.0 ** -22)
    lb = full['leaf_boxes']
    real = np.all(lb[:, :, :3] <= lb[:, :, 3:], axis=2)
    assert lb.shape == (info['tree_leaves'], 4, 6) and real.sum() == info['references']
    assert np.all(real.sum(axis=1) >= 2) and np.all(real.sum(axis=1) <= 4)
    # a parent's box holds its children's; a level-0 box holds its leaf's face boxes
    fb = full['family_boxes']
    for l in range(1, len(ln)):
        for i in range(ln[l]):
            ch = fb[l - 1][4 * i:4 * i + 4]
            ch = ch[ch[:, 0] <= ch[:, 3]]
            assert np.all(fb[l][i, :3] <= ch[:, :3].min(axis=0)) and np.all(fb[l][i, 3:] >= ch[:, 3:].max(axis=0))
    for i in range(ln[0]):
        ch = lb[i][real[i]]
        assert np.all(fb[0][i, :3] <= ch[:, :3].min(axis=0)) and np.all(fb[0][i, 3:] >= ch[:, 3:].max(axis=0))
    whole = shape_of(name, monkeypatch, split=0)
    assert whole['references'] == F and whole['NG'] == 1
    if name == 'longwire':
        assert info['references'] > 2 * F


def test_tree_shapes_cover_padding():
    """Among the three meshes: a level whose node count is no multiple of four (padding nodes, which only the slab test keeps rays
    out of) and leaves with empty slots."""
    infos = [shape_of(name) for name in MESHES]
    assert any(c % 4 for info in infos for c in info['level_nodes'])
    assert any(info['pad_slots'] > 0 for info in infos)


def check_cast(R, tc, fc, what, bits=True):
    """(tc, fc) of an engine against the reference on every ray of R: fc in the admissible set everywhere and the reference's own on
    decided rays (on an exact tie the lowest face index), hit or miss as the reference says, tc = inf on misses and the
    reference's t on hits -- bit for bit (see test_tree_edges); the deviation is recorded per family either way."""
    n = fc.shape[0]
    assert n == R['fc'].shape[0]
    bad = [i for i in range(n) if int(fc[i]) not in R['adm'][i]]
    assert not bad, (what, bad[:10])
    dec, hit = R['decided'], R['hit']
    assert np.array_equal(fc[dec], R['fc'][dec]), (what, np.nonzero(dec & (fc != R['fc']))[0][:10])
    assert np.array_equal(fc >= 0, hit) and np.all(np.isinf(tc[~hit])) and np.all(tc[~hit] > 0), what
    for k, i in sorted(R['fam'].items()):
        h = i[hit[i]]
        assert rel_err(tc[h], R['tc'][h], tag='%s %s' % (what, k), bound=0 if bits else 1e-12, depth=2) < 1e-12, (what, k)
        if bits:
            assert np.array_equal(tc[h], R['tc'][h]), (what, k)


@pytest.mark.parametrize('name', MESHES)
def test_tree_edges(name):
    """Every family through the tree walk against the all-faces float64 reference (the oracle's arithmetic, test_tree_edges_host.py).
    The bound on t is the project's 1e-12 (test_gpu_edges.py); the face arithmetic is the reference's statement by statement under
    fp contract(off), every family measured a deviation of 0 on the MI355X (profiles/tree_edge_margins.txt), so t is held to bit
    equality.  No ray is left out: "decided" only selects where the facet must be the reference's own."""
    eng = tree_engine(name)
    R = all_rays(name, eng)
    assert R['nboxes'] >= 30 and R['fam']['boxwall'].shape[0] >= 1000
    bw = R['fam']['boxwall']
    assert R['hit'][bw].sum() >= 200 and (~R['hit'][bw]).sum() >= 200        # starts inside the solid and outside
    print('%s: %d rays, undecided share %.4f; per family: %s' % (name, R['fc'].shape[0], 1.0 - R['decided'].mean(), ', '.join(
        '%s %.4f' % (k, 1.0 - R['decided'][i].mean()) for k, i in R['fam'].items())))
    xc, tc, fc = eng.find_boundary(R['x'], R['v'])
    eng.close()
    check_cast(R, tc, fc, 'tree')


@pytest.mark.parametrize('name', MESHES)
def test_tree_builds_agree(name, monkeypatch):
    """The same rays through the default tree, the tree of whole faces (NK_TREE_SPLIT=0) and the plane sweep (NK_NO_TREE=1).  The two
    trees differ only in the filter in front of the same face code: tc and fc bit for bit on every ray.  The sweep orders its
    candidates otherwise: bit for bit on decided rays, an admissible facet and the reference's t elsewhere."""
    eng = tree_engine(name)
    R = all_rays(name, eng)
    out = [eng.find_boundary(R['x'], R['v'])]
    shape = [eng.tree_info()]
    eng.close()
    for var, val in (('NK_TREE_SPLIT', '0'), ('NK_NO_TREE', '1')):
        monkeypatch.setenv(var, val)
        eng = tree_engine(name)
        out.append(eng.find_boundary(R['x'], R['v']))
        shape.append(eng.tree_info())
        eng.close()
        monkeypatch.delenv(var)
    assert [s['NG'] for s in shape] == [1, 1, 0] and shape[1]['references'] == FACES[name] <= shape[0]['references']
    (_, t0, f0), (_, t1, f1), (_, t2, f2) = out
    assert np.array_equal(f0, f1) and np.array_equal(t0, t1)
    dec = R['decided']
    assert np.array_equal(f0[dec], f2[dec]) and np.array_equal(t0[dec], t2[dec])
    check_cast(R, t2, f2, 'sweep')


@pytest.mark.parametrize('name', ['wire72', 'star'])
def test_tree_skip(name):
    """nk_tree_skip through Engine.find_boundary(x, v, from_facet): starts on a cap flying inwards, a hair off it on either side,
    grazing and outward, on its rim, and under wrong names.  The skip never changes a result; it engages where the NumPy
    restatement says (wherever the two sides of its inequality differ by more than 1e-5 relative: the device forms dk with fused
    products and the factor 1.000001 is the rule's own margin), on most inward rays, on no ray that hits the named cap itself, on
    no wrong name."""
    g = EC.tree_mesh(name)
    S = EC.skip_families(name)
    x, v, ff, fam = S['x'], S['v'], S['from_facet'], S['fam']
    eng = tree_engine(name)
    xc, tc, fc = eng.find_boundary(x, v)
    xs, ts, fs, sk = eng.find_boundary(x, v, from_facet=ff)
    _, tn, fn_, skn = eng.find_boundary(x, v, from_facet=np.full(x.shape[0], -1))
    eng.close()
    assert np.array_equal(fs, fc) and np.array_equal(ts, tc) and np.array_equal(xs, xc, equal_nan=True)
    assert np.array_equal(fn_, fc) and np.array_equal(tn, tc) and not skn.any()
    assert set(np.unique(sk)) <= {0, 1}
    want, lhs, rhs = EC.tree_skip_rule(g, ff, x, v)
    clear = np.abs(lhs - rhs) > 1e-5 * np.maximum(np.abs(lhs), np.abs(rhs))
    assert clear.mean() > 0.9
    assert np.array_equal(sk[clear] == 1, want[clear]), np.nonzero(clear & ((sk == 1) != want))[0][:10]
    assert sk[fam['a']].mean() > 0.5
    assert not sk[fc == ff].any()
    assert not sk[fam['e']].any()
    # the families reach both sides of the rule
    for k in 'bc':
        assert sk[fam[k]].any() and not sk[fam[k]].all(), k
    assert sk[fam['d']].mean() > 0.5
    # against the all-faces reference as well: the starts on a cap are decided rays
    ref = EC.cached(('skip_ref', name), lambda: EC.all_faces_cast(g, x, v))
    dec, _ = EC.decided(ref)
    assert all(int(fs[i]) in ref['adm'][i] for i in range(fs.shape[0])) and np.array_equal(fs[dec], ref['fc'][dec])
    assert np.array_equal(ts[ref['hit']], ref['tc'][ref['hit']]) and np.all(np.isinf(ts[~ref['hit']]))


def test_find_boundary_from_on_an_lds_mesh():
    """On a mesh whose tables sit in LDS there is no tree and nothing to skip: the same results, skipped = 0 everywhere."""
    from test_gpu_edges import mesh_engine
    g = EC.lds_mesh('cyl')
    L = EC.lds_families('cyl')
    eng = mesh_engine(g)
    assert eng.tree_info()['NG'] == 0 and eng.tree_info(boxes=True)['tree_leaves'] == 0
    xc, tc, fc = eng.find_boundary(L['x'], L['v'])
    rng = np.random.default_rng(3)
    ff = rng.integers(-1, len(g['bound_cond']) + 1, size=fc.shape[0])
    xs, ts, fs, sk = eng.find_boundary(L['x'], L['v'], from_facet=ff)
    eng.close()
    assert np.array_equal(fs, fc) and np.array_equal(ts, tc) and np.array_equal(xs, xc, equal_nan=True) and not sk.any()
