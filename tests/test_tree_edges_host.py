"""The edge inputs of the face-tree tests are what they claim to be -- checked on the CPU, with the all-faces reference, the
package's Mesh.find_boundary and the oracle alone, so that test_gpu_tree_edges.py cannot pass for want of a tie, a miss, a sliver
hit or a ray whose facet is decided: the reference names the facet of both other evaluations on every decided ray, most rays are
decided, every family is there, and the NumPy restatement of the facet skip says what nk_tree_skip's comment promises."""
import numpy as np
import pytest

import edge_cases as EC
from util import rel_err
from test_edge_cases_host import oracle_cast

MESHES = ['wire72', 'star', 'longwire']
# decided share of all rays, measured on the reference alone: 0.963, 0.989, 0.969 (lowest single family: `edge` on wire72, 0.824)
MIN_DECIDED = 0.9


@pytest.mark.parametrize('name', MESHES)
def test_tree_meshes_are_cast_through_the_tree(name):
    g = EC.tree_mesh(name)
    F = np.asarray(g['face_normals']).shape[0]
    assert F > 256                                            # NK_LDS_FACES
    assert F == {'wire72': 288, 'star': 576, 'longwire': 288}[name]
    caps = EC.cap_facets(g)
    nf = np.bincount(np.asarray(g['face_facets'], dtype=int))
    assert len(caps) == 2 and all(nf[c] >= 16 for c in caps) and nf[np.setdiff1d(np.arange(nf.shape[0]), caps)].max() < 16
    if name == 'longwire':                                    # side triangles of ~13 A x 60 000 A
        V = np.asarray(g['vertices'], dtype=float)[np.asarray(g['faces'], dtype=int)[EC.side_faces(g)]]
        ext = np.sort(np.stack([np.linalg.norm(V[:, (k + 1) % 3] - V[:, k], axis=1) for k in range(3)]), axis=0)
        assert ext[0].max() < 14.0 and ext[2].min() >= 60000.0


@pytest.mark.parametrize('name', MESHES)
def test_reference_against_package_and_oracle(name):
    """all_faces_cast names the facet of Mesh.find_boundary and of nko_find_boundary on every decided ray (elsewhere theirs lies
    in the admissible set), hit or miss agrees everywhere, t to 1e-12."""
    ct = EC.tree_case(name)
    g = ct['mesh']
    L = EC.tree_families(name)
    ref = L['ref']
    dec, _ = EC.decided(ref)
    hit = ref['hit']
    with np.errstate(all='ignore'):
        _, tp, fp = ct['geo'].mesh.find_boundary(L['x'].copy(), L['v'].copy())
    to, fo = oracle_cast(g, L['x'], L['v'])
    for who, t, f in (('package', tp, np.asarray(fp).astype(int)), ('oracle', to, fo)):
        assert np.array_equal(f[dec], ref['fc'][dec]), who
        assert all(int(f[i]) in ref['adm'][i] for i in range(f.shape[0])), who
        assert np.array_equal(f >= 0, hit) and np.all(np.isinf(t[~hit])), who
        assert rel_err(t[hit], ref['tc'][hit]) < 1e-12, who
    assert np.array_equal(to, ref['tc'])                      # the reference is the oracle's arithmetic, statement by statement


@pytest.mark.parametrize('name', MESHES)
def test_tree_families_are_what_they_claim(name):
    g = EC.tree_mesh(name)
    L = EC.tree_families(name)
    ref, fam = L['ref'], L['fam']
    dec, tie = EC.decided(ref)
    n = L['x'].shape[0]
    print('%s: %d rays, decided %.3f, %d exact face ties, %d misses; per family: %s' % (
        name, n, dec.mean(), tie.sum(), (~ref['hit']).sum(), ', '.join('%s %.3f' % (k, dec[i].mean()) for k, i in fam.items())))
    assert dec.mean() >= MIN_DECIDED
    assert tie.sum() > 500 and (~ref['hit']).sum() > 100
    want = ['generic', 'surface', 'outside', 'axis', 'diagonal', 'edge', 'vertex', 'speed', 'tiny', 'far'] + (['sliver'] if name == 'longwire' else [])
    assert sorted(fam) == sorted(want) and all(fam[k].shape[0] >= 100 for k in want)
    assert np.array_equal(np.sort(np.concatenate(list(fam.values()))), np.arange(n))          # no ray outside every family
    # the first 4038 / 6630 rays are lds_families' generator on this mesh, unchanged
    x0, v0, fam0, _ = EC.ray_families(g, EC.TREE_SEED, EC.TREE_NGEN, False)
    assert np.array_equal(L['x'][:x0.shape[0]], x0) and np.array_equal(L['v'][:x0.shape[0]], v0)
    # speed: the four magnitudes, the directions of `generic`
    sp = np.linalg.norm(L['v'][fam['speed']], axis=1)
    for k, s in enumerate(EC.SPEEDS):
        assert rel_err(sp[k::4], np.full(sp[k::4].shape[0], s)) < 1e-15
    assert ref['hit'][fam['speed']].all() and np.array_equal(ref['fc'][fam['speed']], ref['fc'][fam['generic']])
    # tiny: one component +-40, the others at most 1e-6 and every value of either sign there; all hit (the ray is as good as axial)
    vt = L['v'][fam['tiny']]
    big = np.abs(vt) == 40.0
    assert np.all(big.sum(axis=1) == 1) and np.abs(vt[~big]).max() == 1e-6 and ref['hit'][fam['tiny']].all()
    small = vt[~big]
    for t in EC.TINY:
        for sg in (False, True):
            assert np.any((np.abs(small) == t) & (np.signbit(small) == sg)), (t, sg)
    if name == 'longwire':
        i = fam['sliver']
        side = EC.side_faces(g)
        faces_hit = np.intersect1d(ref['face'][i], side)
        assert faces_hit.shape[0] >= 20
        # ... at points spread over the whole length, and some after thousands of angstrom of flight
        z = (L['x'][i] + ref['tc'][i][:, None] * L['v'][i])[:, 2]
        zs = z[np.isin(ref['face'][i], side)]
        assert zs.min() < 0.02 * 60000.0 and zs.max() > 0.98 * 60000.0
        assert (ref['tc'][i] * np.linalg.norm(L['v'][i], axis=1) > 2000.0).sum() >= 50
    # far: starts 1e3 .. 1e6 A from the targets, most of them hits, a good share of them ending on two faces at once
    i = fam['far']
    d = ref['tc'][i] * 40.0
    assert ref['hit'][i].mean() > 0.9 and np.nanmin(d[ref['hit'][i]]) > 500.0 and (d[ref['hit'][i]] > 1e5).sum() >= 50
    assert ref['close2'][i].sum() >= 100
    x, v = EC.subtiny_rays(g)
    assert x.shape[0] == 20 and np.abs(v).max() < 1e-30 and np.all((v != 0.0).sum(axis=1) >= 2)


@pytest.mark.parametrize('name', ['wire72', 'star'])
def test_skip_rule_restated(name):
    """tree_skip_rule (nk_tree_skip in NumPy) says "skip" for starts on a cap flying inwards, "no" for side facets whatever the
    ray, and "no" for starts a distance delta off the cap with delta / |v.n| >= tol: there the cap's own t may reach tol and
    the cap could be hit."""
    g = EC.tree_mesh(name)
    S = EC.skip_families(name)
    x, v, ff, fam = S['x'], S['v'], S['from_facet'], S['fam']
    fn = np.asarray(g['facets_normal'], dtype=float)
    dn, dk = EC.facet_skip_tables(g)
    for c in S['caps']:
        assert dn[c] < 1e-12 and dk[c] < 1e-9
    sides = np.setdiff1d(np.arange(fn.shape[0]), S['caps'])
    assert np.all(dn[sides] == 1e300)
    skip, lhs, rhs = EC.tree_skip_rule(g, ff, x, v)
    a = fam['a']
    vn = np.abs(np.sum(v[a] * fn[ff[a]], axis=1))
    assert a.shape[0] == 3000 and skip[a][vn >= 1.0].all() and skip[a].mean() > 0.9
    assert not skip[fam['e']].any()
    assert not EC.tree_skip_rule(g, np.full(a.shape[0], sides[0]), x[a], v[a])[0].any()
    b = fam['b']
    nb = fn[ff[b]]
    delta = np.abs(np.sum((x[b] - np.asarray(g['facet_centroid'], dtype=float)[ff[b]]) * nb, axis=1))
    ratio = delta / np.abs(np.sum(v[b] * nb, axis=1))
    far = ratio >= EC.TOL
    assert far.sum() >= 0.3 * b.shape[0] and not skip[b][far].any()
    assert skip[b][ratio < 0.45 * EC.TOL].mean() > 0.9 and (ratio < 0.45 * EC.TOL).sum() >= 0.1 * b.shape[0]
    # grazing and outward rays are in the family, and every sub-family is there
    assert sorted(fam) == ['a', 'b', 'c', 'd', 'e'] and all(fam[k].shape[0] >= 100 for k in fam)
    c = fam['c']
    assert (np.sum(v[c] * fn[ff[c]], axis=1) > 0).sum() >= 100 and (np.sum(v[c] * fn[ff[c]], axis=1) == 0).sum() >= 50
