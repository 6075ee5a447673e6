"""Inputs at the edges of the device lookups, and exact references for them, shared by test_edge_cases_host.py (CPU) and
test_gpu_edges.py (GPU): rays that tie or nearly tie between box walls, start on walls or a hair from them; rays through edges,
vertices and quad diagonals of the small meshes; points on and next to slice edges, centres and grid bisectors; temperatures
on the nodes and window borders of the lifetime table.

At these inputs engine and oracle may legitimately name different walls or slices: the oracle picks a wall by rounded
quotients and the engine by cross products, the oracle a slice by rounded 3-D squared distances and the engine by a 1-D
comparison.  Who is right is decided here, in exact rational arithmetic on the doubles (fractions.Fraction)."""
import math
from fractions import Fraction as Fr

import numpy as np

from util import golden, sub, case_from_args

TOL = 1e-10                    # Mesh.tol
U = Fr(1, 2 ** 53)             # unit roundoff
NEAR = Fr(1, 2 ** 50)          # two walls whose exact t differ by less than this (relative) are a near-tie: either may be named
DBL_MAX = Fr(np.finfo(float).max)

COMMON_ARGS = ['--poscar_file', 'POSCAR', '--hdf_file', 'synthetic', '--temp_interp', 'linear', '--timestep', '1',
               '--energy_normal', 'mean', '--particles', 'total', '30000']
# a cuboid with three unequal sides that are no doubles: periodic along x, reservoirs on the y walls, rough z walls
CUBOID_ARGS = ['--geometry', 'box', '--dimensions', '123.4567', '97.531', '151.2345', '--subvolumes', 'slice', '5', '1',
               '--bound_pos', 'relative', '.5', '0', '.5', '.5', '1', '.5', '.5', '.5', '0', '.5', '.5', '1',
               '--bound_cond', 'T', 'T', 'R', 'R', 'P', '--bound_values', '302', '298', '5', '5',
               '--connect_pos', 'relative', '0', '.5', '.5', '1', '.5', '.5']
NONCONVEX_ARGS = {
    'corrugated': ['--geometry', 'corrugated', '--dimensions', '80', '60', '35', '10', '5', '--subvolumes', 'slice', '8', '2',
                   '--bound_pos', 'relative', '0.5', '0.5', '0', '0.5', '0.5', '1', '--bound_cond', 'T', 'T', 'R',
                   '--bound_values', '302', '298', '5'],
    'castle': ['--geometry', 'castle', '--dimensions', '90', '40', '70', '45', '8', '5', '1', '--subvolumes', 'slice', '8', '2',
               '--bound_pos', 'relative', '0.5', '0.5', '0', '0.5', '0.5', '1', '--bound_cond', 'T', 'T', 'R',
               '--bound_values', '302', '298', '5'],
}

_CACHE = {}


def cached(key, make):
    """References are computed once per process and shared by the tests; callers must not modify them."""
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def ulp_shift(x, k):
    """x moved by k units in the last place (k of either sign), across zero if need be."""
    x = np.array(x, dtype=float, copy=True)
    out = x.copy()
    for _ in range(abs(int(k))):
        out = np.nextafter(out, np.inf if k > 0 else -np.inf)
    return out


def hi_lo(q):
    """An exact rational as the double it rounds to plus the remainder (the arguments of util.ulp_err)."""
    if q is None:
        return math.nan, 0.0
    hi = float(q)
    return hi, float(q - Fr(hi))


# ------------------------------------------------------------------------------------------ meshes
def permuted_mesh(g, face_perm, facet_perm):
    """The same surface with its faces listed in another order (new face i = old face face_perm[i]) and its facets renamed
    (old facet f becomes facet_perm[f]): the tables of Engine.set_mesh / oracle make_mesh."""
    fp, cp = np.asarray(face_perm), np.asarray(facet_perm)
    inv_f = np.argsort(fp)
    out = dict(g)
    for k in ('faces', 'face_normals', 'face_k', 'face_basis_matrix', 'face_origins', 'face_areas'):
        out[k] = np.ascontiguousarray(np.asarray(g[k])[fp])
    out['face_bounds'] = np.ascontiguousarray(np.asarray(g['face_bounds'])[:, fp])
    out['face_facets'] = cp[np.asarray(g['face_facets'])[fp]]
    inv_c = np.argsort(cp)
    for k in ('facets_normal', 'facet_centroid', 'bound_cond'):
        out[k] = np.ascontiguousarray(np.asarray(g[k])[inv_c])
    lists = g['facets'] if 'facets' in g else np.split(np.asarray(g['facets_flat']), np.cumsum(g['facets_len'])[:-1])
    out.pop('facets_flat', None), out.pop('facets_len', None)
    out['facets'] = [np.sort(inv_f[np.asarray(lists[int(c)], dtype=int)]) for c in inv_c]
    out['connected_facets'] = cp[np.asarray(g.get('connected_facets', np.zeros((0, 2))), dtype=int).reshape(-1, 2)]
    return out


def box_mesh(name):
    """'cube': golden box200ttp.  'cuboid': CUBOID_ARGS through case_from_args, faces and facets then renumbered so that the
    maps wall -> facet and wall -> first face differ from the cube's (the box primitive lists every box the same way)."""
    def make():
        if name == 'cube':
            return sub(golden('mesh'), 'box200ttp')
        g = case_from_args(CUBOID_ARGS + COMMON_ARGS)['mesh']
        return permuted_mesh(g, [10, 11, 6, 7, 2, 3, 8, 9, 0, 1, 4, 5], [3, 5, 0, 4, 2, 1])
    return cached(('box_mesh', name), make)


def lds_mesh(name):
    def make():
        if name in ('box200ttp', 'cyl'):
            return sub(golden('mesh'), name)
        return case_from_args(NONCONVEX_ARGS[name] + COMMON_ARGS)['mesh']
    return cached(('lds_mesh', name), make)


def box_walls(g):
    """Walls w = 2 a + (normal +e_a): position (lo = k of the wall with normal -e_a, hi = -k of the other: NkBoxWalls), facet and
    lowest face index, from the face tables as nk_set_mesh reads them."""
    n, k, ff = np.asarray(g['face_normals']), np.asarray(g['face_k']), np.asarray(g['face_facets'])
    pos, facet, face0 = np.zeros(6), -np.ones(6, dtype=int), np.full(6, 1 << 30)
    for f in range(n.shape[0]):
        a = int(np.argmax(np.abs(n[f])))
        assert abs(n[f, a]) == 1.0 and np.count_nonzero(n[f]) == 1
        w = 2 * a + (1 if n[f, a] > 0 else 0)
        pos[w] = -k[f] if n[f, a] > 0 else k[f]
        assert facet[w] in (-1, ff[f])
        facet[w], face0[w] = int(ff[f]), min(face0[w], f)
    return dict(pos=pos, facet=facet, face0=face0, lo=pos[0::2].copy(), hi=pos[1::2].copy())


# ------------------------------------------------------------------------- exact box casts
def _pick(cands, key, W):
    """cands: [(wall, value)]; the best value by `key` (min or max), its exact ties, the near-ties within NEAR."""
    best = key(v for _, v in cands)
    tied = [w for w, v in cands if v == best]
    adm = [w for w, v in cands if abs(v - best) <= NEAR * best]
    wbest = min(tied, key=lambda w: W['face0'][w])
    return dict(wall=wbest, facet=int(W['facet'][wbest]), value=best, tie=len(tied) > 1, adm={int(W['facet'][w]) for w in adm},
                per_facet={int(W['facet'][w]): v for w, v in cands})


MISS = dict(wall=-1, facet=-1, value=None, tie=False, adm={-1}, per_facet={})


def exact_next_hit(W, x, v, tol=TOL):
    """Mesh.find_boundary on a box, exactly: per wall the ray flies towards t = (wall - x_a) / v_a; admissible when
    t >= tol and finite in double; the smallest wins, among equal rationals the wall with the lowest face index."""
    cands = []
    for a in range(3):
        if v[a] == 0.0 or not math.isfinite(v[a]):
            continue
        w = 2 * a + (1 if v[a] > 0 else 0)
        t = (Fr(float(W['pos'][w])) - Fr(float(x[a]))) / Fr(float(v[a]))
        if t > 0 and t >= Fr(tol) and t <= DBL_MAX:
            cands.append((w, t))
    return _pick(cands, min, W) if cands else MISS


def exact_first_hit(W, x, v):
    """The wall a particle at its end-of-step position x crossed first: among the walls it lies beyond and flies towards, the
    largest (distance beyond) / |v_a|.  value = that quotient (n_timesteps = -value / dt)."""
    cands = []
    for a in range(3):
        if v[a] > 0 and x[a] > W['hi'][a]:
            cands.append((2 * a + 1, (Fr(float(x[a])) - Fr(float(W['hi'][a]))) / Fr(float(v[a]))))
        elif v[a] < 0 and x[a] < W['lo'][a]:
            cands.append((2 * a, (Fr(float(W['lo'][a])) - Fr(float(x[a]))) / -Fr(float(v[a]))))
    return _pick(cands, max, W) if cands else MISS


def exact_all(fn, W, x, v, **kw):
    return [fn(W, x[i], v[i], **kw) for i in range(x.shape[0])]


# ------------------------------------------------------------------------- ray families, box
EDGES = [(a, sa, b, sb) for a in range(3) for b in range(a + 1, 3) for sa in (0, 1) for sb in (0, 1)]
CORNERS = [(sx, sy, sz) for sx in (0, 1) for sy in (0, 1) for sz in (0, 1)]


def _inside(W, rng, n, margin=0.02):
    lo, hi = W['lo'] + 0.0, W['hi']
    return lo + (margin + (1 - 2 * margin) * rng.random((n, 3))) * (hi - lo)


def box_next_families(name):
    """Families (a) - (f) of next-hit rays on a box mesh: {family: (x, v)}."""
    def make():
        W = box_walls(box_mesh(name))
        rng = np.random.default_rng(1234 if name == 'cube' else 4321)
        lo, hi = W['lo'] + 0.0, W['hi']
        fam = {}
        # (a) generic interior rays
        fam['a'] = (_inside(W, rng, 4096), rng.normal(size=(4096, 3)) * 40.0)
        # (b) starts exactly on a wall, an edge or a corner, flying inwards; sliding (v_a = 0.0, -0.0) along a wall they stand on
        X, V = [], []
        for cell in np.ndindex(3, 3, 3):
            on = [a for a in range(3) if cell[a] != 1]
            if not on:
                continue
            variants = [{}] + [{a: z} for a in on for z in (0.0, -0.0)] + ([{a: (0.0 if i else -0.0) for i, a in enumerate(on)}] if len(on) > 1 else [])
            for var in variants:
                if len(var) == 3:
                    continue
                for _ in range(3):
                    x, v = _inside(W, rng, 1)[0], rng.normal(size=3) * 40.0
                    for a in on:
                        x[a] = lo[a] if cell[a] == 0 else hi[a]
                        v[a] = abs(v[a]) if cell[a] == 0 else -abs(v[a])
                    for a, z in var.items():
                        v[a] = z
                    if np.all(v == 0.0):
                        continue
                    X.append(x), V.append(v)
        fam['b'] = (np.array(X), np.array(V))
        # (c) starts at distance d from the wall they fly towards, d / |v_a| = tol / 4 (the wall is skipped) and 4 tol (it is hit)
        X, V, R = [], [], []
        for w in range(6):
            for ratio in (0.25, 4.0):
                for _ in range(16):
                    a, up = w // 2, w % 2
                    x, v = _inside(W, rng, 1, 0.2)[0], rng.normal(size=3) * 40.0
                    v[a] = (1 if up else -1) * (10.0 + abs(v[a]))
                    d = ratio * TOL * abs(v[a])
                    x[a] = hi[a] - d if up else lo[a] + d
                    X.append(x), V.append(v), R.append(ratio)
        fam['c'] = (np.array(X), np.array(V))
        fam['c_ratio'] = np.array(R)
        # (d) exact ties: starts 32 A in front of the two (edges) or three (corners) walls aimed at -- the subtraction is exact --
        # velocity components 0 or +-2^e, three magnitudes
        X, V = [], []
        for e in (-3, 2, 9):
            s = 2.0 ** e
            for (a, sa, b, sb) in EDGES:
                x, v = 0.5 * (lo + hi), np.zeros(3)
                for ax, sg in ((a, sa), (b, sb)):
                    x[ax] = hi[ax] - 32.0 if sg else lo[ax] + 32.0
                    v[ax] = s if sg else -s
                X.append(x), V.append(v)
            for c in CORNERS:
                x = np.array([hi[ax] - 32.0 if c[ax] else lo[ax] + 32.0 for ax in range(3)])
                X.append(x), V.append(np.array([s if c[ax] else -s for ax in range(3)]))
        fam['d'] = (np.array(X), np.array(V))
        # (e) near-ties: from random interior points towards random points of the twelve edges and the eight corners, velocities
        # rounded to double
        X, V = [], []
        for i in range(1200):
            x = _inside(W, rng, 1, 0.05)[0]
            tgt = _inside(W, rng, 1, 0.05)[0]
            if i % 5 == 4:
                c = CORNERS[(i // 5) % 8]
                tgt = np.array([hi[ax] if c[ax] else lo[ax] for ax in range(3)])
            else:
                a, sa, b, sb = EDGES[i % 12]
                tgt[a], tgt[b] = (hi[a] if sa else lo[a]), (hi[b] if sb else lo[b])
            X.append(x), V.append((tgt - x) * 0.125)
        fam['e'] = (np.array(X), np.array(V))
        # (f) misses: v = 0, a velocity so small that t overflows; and v along one axis from the wall it leaves: the far wall
        c = 0.5 * (lo + hi)
        X = [c, c, c, c, c, c]
        V = [[0.0, 0.0, 0.0], [-0.0, 0.0, -0.0], [5e-324, 0.0, 0.0], [0.0, -1e-310, -0.0], [0.0, 0.0, 2e-308], [-5e-324, 5e-324, 5e-324]]
        nmiss = len(X)
        for w in range(6):
            a, up = w // 2, w % 2
            for z in (0.0, -0.0):
                x, v = _inside(W, rng, 1)[0], np.array([z, -z, z])
                x[a] = hi[a] if up else lo[a]
                v[a] = -37.5 if up else 37.5
                X.append(x), V.append(v)
        fam['f'] = (np.array(X, dtype=float), np.array(V, dtype=float))
        fam['f_nmiss'] = nmiss
        return fam
    return cached(('box_next', name), make)


def box_first_families(name):
    """Family (g): end-of-step points for nk_box_out / nk_box_first_hit: {sub-family: (x, v)}."""
    def make():
        W = box_walls(box_mesh(name))
        rng = np.random.default_rng(99 if name == 'cube' else 77)
        lo, hi = W['lo'] + 0.0, W['hi']
        fam = {}

        def beyond(axes_signs, mode):
            x, v = _inside(W, rng, 1)[0], rng.normal(size=3) * 40.0
            for a, sg in axes_signs:
                wall = hi[a] if sg else lo[a]
                out = 1.0 if sg else -1.0
                if mode == 'beyond':
                    x[a] = wall + out * (0.01 + 5.0 * rng.random())
                elif mode == 'on':
                    x[a] = wall
                elif mode == 'next':
                    x[a] = np.nextafter(wall, out * np.inf)
                elif mode == 'away':
                    x[a] = wall + out * (0.01 + 5.0 * rng.random())
                v[a] = out * (1.0 + abs(v[a])) * (-1.0 if mode == 'away' else 1.0)
            return x, v
        for k in (1, 2, 3):
            X, V = [], []
            for _ in range(64):
                axes = rng.permutation(3)[:k]
                x, v = beyond([(int(a), int(rng.integers(2))) for a in axes], 'beyond')
                X.append(x), V.append(v)
            fam['beyond%d' % k] = (np.array(X), np.array(V))
        for mode in ('on', 'next', 'away'):
            X, V = [], []
            for w in range(6):
                for _ in range(6):
                    x, v = beyond([(w // 2, w % 2)], mode)
                    X.append(x), V.append(v)
            fam[mode] = (np.array(X), np.array(V))
        # beyond one wall flown towards and beyond another flown away from: only the first counts
        X, V = [], []
        for (a, sa, b, sb) in EDGES:
            x, v = beyond([(a, sa)], 'beyond')
            x2, v2 = beyond([(b, sb)], 'away')
            x[b], v[b] = x2[b], v2[b]
            X.append(x), V.append(v)
        fam['mixed'] = (np.array(X), np.array(V))
        # exact ties: 1/8 A beyond two or three walls, speed components +-2^e
        X, V = [], []
        for e in (-2, 4):
            s = 2.0 ** e
            for (a, sa, b, sb) in EDGES:
                x, v = 0.5 * (lo + hi), rng.normal(size=3)
                for ax, sg in ((a, sa), (b, sb)):
                    x[ax] = hi[ax] + 0.125 if sg else lo[ax] - 0.125
                    v[ax] = s if sg else -s
                X.append(x), V.append(v)
            for c in CORNERS:
                X.append(np.array([hi[ax] + 0.125 if c[ax] else lo[ax] - 0.125 for ax in range(3)]))
                V.append(np.array([s if c[ax] else -s for ax in range(3)]))
        fam['ties'] = (np.array(X), np.array(V))
        return fam
    return cached(('box_first', name), make)


# --------------------------------------------------------------- all-faces float64 cast, general meshes
def plane_times(g, x, v, tol=TOL):
    """t of every distinct plane as the engine groups them (equal normal and k; the first face of each stands for it), inf where
    it is not admissible (t >= tol, finite); and the plane of every face."""
    n_, k_ = np.asarray(g['face_normals'], dtype=float), np.asarray(g['face_k'], dtype=float)
    key = np.ascontiguousarray(np.concatenate([n_, k_[:, None]], axis=1) + 0.0).view(np.uint64).reshape(-1, 4)      # (-0.0 == 0.0)
    _, first, inv = np.unique(key, axis=0, return_index=True, return_inverse=True)
    n_, k_ = n_[first], k_[first]
    with np.errstate(all='ignore'):
        num = (x[:, 0:1] * n_[:, 0] + x[:, 1:2] * n_[:, 1]) + x[:, 2:3] * n_[:, 2]
        den = (v[:, 0:1] * n_[:, 0] + v[:, 1:2] * n_[:, 1]) + v[:, 2:3] * n_[:, 2]
        t = -(num + k_) / den
        t = np.where((t >= tol) & np.isfinite(t), t, np.inf)
    return t, np.asarray(inv).reshape(-1)


def all_faces_cast(g, x, v, tol=TOL, chunk=1024):
    """_all_faces_block on `chunk` rays at a time (it holds n x F x 3 arrays); every ray is evaluated on its own, so the result
    does not depend on the chunk."""
    x, v = np.asarray(x, dtype=float), np.asarray(v, dtype=float)
    if x.shape[0] <= chunk:
        return _all_faces_block(g, x, v, tol)
    parts = [_all_faces_block(g, x[a:a + chunk], v[a:a + chunk], tol) for a in range(0, x.shape[0], chunk)]
    return {k: (sum((q[k] for q in parts), []) if k == 'adm' else np.concatenate([q[k] for q in parts])) for k in parts[0]}


def _all_faces_block(g, x, v, tol=TOL):
    """Mesh.find_boundary in float64 with the arithmetic of oracle/nk_oracle.c find_boundary_one (products summed left to
    right, no fused multiply-adds, barycentric coordinates by Cramer's rule), returning EVERY passing face:
    T [n, F] (inf where a face does not pass), and per ray tc, the first face of the minimum, its facet, the admissible set of
    facets (passing faces with t <= tc (1 + 2^-50)), whether two faces pass within 1e-12 of tc (`close2`); and, per distinct plane as the engine groups them (bitwise equal normal
    and k), whether the nearest admissible plane has no passing face (`noface`) and whether two planes tie for the smallest
    t (`planetie`)."""
    n_, k_ = np.asarray(g['face_normals'], dtype=float), np.asarray(g['face_k'], dtype=float)
    fb = np.asarray(g['face_bounds'], dtype=float)
    A, o = np.asarray(g['face_basis_matrix'], dtype=float), np.asarray(g['face_origins'], dtype=float)
    ff = np.asarray(g['face_facets']).astype(int)
    x, v = np.asarray(x, dtype=float), np.asarray(v, dtype=float)
    with np.errstate(all='ignore'):
        num = (x[:, 0:1] * n_[:, 0] + x[:, 1:2] * n_[:, 1]) + x[:, 2:3] * n_[:, 2]
        den = (v[:, 0:1] * n_[:, 0] + v[:, 1:2] * n_[:, 1]) + v[:, 2:3] * n_[:, 2]
        t = -(num + k_) / den
        valid = (t >= tol) & np.isfinite(t)
        tt = np.where(valid, t, 0.0)
        c = x[:, None, :] + tt[:, :, None] * v[:, None, :]
        inb = np.all(c >= fb[0][None] - tol, axis=2) & np.all(c <= fb[1][None] + tol, axis=2)
        b = c - o[None]
        a00, a01, a02, a10, a11, a12, a20, a21, a22 = (A[:, i, j] for i in range(3) for j in range(3))
        det = a00 * (a11 * a22 - a12 * a21) - a01 * (a10 * a22 - a12 * a20) + a02 * (a10 * a21 - a11 * a20)
        b0, b1, b2 = b[..., 0], b[..., 1], b[..., 2]
        u = (b0 * (a11 * a22 - a12 * a21) - a01 * (b1 * a22 - a12 * b2) + a02 * (b1 * a21 - a11 * b2)) / det
        w = (a00 * (b1 * a22 - a12 * b2) - b0 * (a10 * a22 - a12 * a20) + a02 * (a10 * b2 - b1 * a20)) / det
        z = 1.0 - (u + w)
        bary = (u >= -tol) & (u <= 1 + tol) & (w >= -tol) & (w <= 1 + tol) & (z >= -tol) & (z <= 1 + tol)
    ok = valid & inb & bary
    T = np.where(ok, t, np.inf)
    tc = T.min(axis=1)
    face = np.argmax(T == tc[:, None], axis=1)
    hit = np.isfinite(tc)
    fc = np.where(hit, ff[face], -1)
    adm = []
    for i in range(x.shape[0]):
        adm.append({int(c_) for c_ in ff[T[i] <= tc[i] * (1.0 + 2.0 ** -50)]} if hit[i] else {-1})
    tp, inv = plane_times(g, x, v, tol)
    tpmin = tp.min(axis=1)
    pmin = np.argmin(tp, axis=1)
    planetie = np.isfinite(tpmin) & ((tp == tpmin[:, None]).sum(axis=1) > 1)
    passing_on_pmin = (ok & (inv[None, :] == pmin[:, None])).any(axis=1)
    noface = np.isfinite(tpmin) & ~planetie & ~passing_on_pmin
    with np.errstate(invalid='ignore'):
        close2 = (T <= tc[:, None] * (1.0 + 1e-12)).sum(axis=1) >= 2      # two passing faces at (nearly) the same t: an edge was hit
    return dict(T=T, tc=tc, face=np.where(hit, face, -1), fc=fc, adm=adm, noface=noface, planetie=planetie, hit=hit, close2=close2 & hit)


def sample_inside(g, n, rng):
    """Uniform points in the solid from the mesh's tetrahedra (Mesh.sample_volume)."""
    sv = np.asarray(g['simplices_volumes'], dtype=float)
    s = rng.choice(sv.shape[0], size=n, p=sv / sv.sum())
    pts = np.asarray(g['simplices_points'], dtype=float)[np.asarray(g['simplices'], dtype=int)[s]]
    a = -np.log(rng.random((n, 4, 1)))
    a /= a.sum(axis=1, keepdims=True)
    return np.sum(a * pts, axis=1)


def _shared_edges(g):
    """[(face i, face j, vertex a, vertex b, coplanar)] for every pair of faces that share an edge."""
    faces = np.asarray(g['faces'], dtype=int)
    n_, k_ = np.asarray(g['face_normals']), np.asarray(g['face_k'])
    owner, out = {}, []
    for f in range(faces.shape[0]):
        for e in range(3):
            a, b = sorted((int(faces[f, e]), int(faces[f, (e + 1) % 3])))
            if (a, b) in owner:
                i = owner[(a, b)]
                out.append((i, f, a, b, bool(np.array_equal(n_[i], n_[f]) and k_[i] == k_[f])))
            else:
                owner[(a, b)] = f
    return out


def _aim(rng, target, normal, scale=0.125):
    """A ray towards `target` from a point 0.5 .. 3 A behind it along -normal, a little off to the side; velocity rounded."""
    h = 0.5 + 2.5 * rng.random()
    nrm = normal / np.linalg.norm(normal)
    side = rng.normal(size=3)
    side -= nrm * (side @ nrm)
    x = target - nrm * h + 0.3 * h * rng.random() * side / np.linalg.norm(side)
    return x, (target - x) * scale / h * 8.0


def ray_families(g, seed, ngen, planetie):
    """The ray families of any mesh table dict g: generic interior rays (ngen of them), starts on the surface and outside,
    axis-parallel rays with zeros of either sign, rays through quad diagonals, edges and vertices, and -- `planetie` -- rays with two
    planes tied for the smallest t.  Returns (x, v, {family: index array}) and the generator, for families that follow."""
    rng = np.random.default_rng(seed)
    V_, faces = np.asarray(g['vertices'], dtype=float), np.asarray(g['faces'], dtype=int)
    n_ = np.asarray(g['face_normals'], dtype=float)
    b = np.asarray(g['bounds'], dtype=float)
    X, V, fam = [], [], {}

    def add(key, x, v):
        start = sum(a.shape[0] for a in X)
        X.append(np.atleast_2d(x)), V.append(np.atleast_2d(v))
        fam[key] = np.arange(start, start + X[-1].shape[0])
    add('generic', sample_inside(g, ngen, rng), rng.normal(size=(ngen, 3)) * 40.0)
    # starts on the surface: first hits of other rays
    x0, v0 = sample_inside(g, 400, rng), rng.normal(size=(400, 3)) * 40.0
    r0 = all_faces_cast(g, x0, v0)
    xs = (x0 + r0['tc'][:, None] * v0)[r0['hit']]
    add('surface', xs, rng.normal(size=xs.shape) * 40.0)
    # starts outside: aimed at the body (hits) and away from it or past it (misses)
    xo = b[1] + 7.0 + 20.0 * rng.random((200, 3))
    xo[::2] = b[0] - 7.0 - 20.0 * rng.random((100, 3))
    vo = rng.normal(size=(200, 3)) * 40.0
    vo[:120] = (sample_inside(g, 120, rng) - xo[:120]) * 0.0625
    add('outside', xo, vo)
    # axis-parallel rays, zeros of either sign
    va = np.zeros((240, 3))
    for i in range(240):
        va[i] = [0.0, -0.0, 0.0][i % 3:] + [0.0, -0.0, 0.0][:i % 3]
        va[i, i % 3] = 40.0 if (i // 3) % 2 else -40.0
    add('axis', sample_inside(g, 240, rng), va)
    # through the shared diagonal of two coplanar triangles / an edge between two faces of different planes / a vertex
    edges = _shared_edges(g)
    for key, want, per in (('diagonal', True, 6), ('edge', False, 4)):
        xs_, vs_ = [], []
        count = sum(1 for e in edges if e[4] == want)
        per = max(per, -(-120 // max(count, 1)))                 # at least 120 rays per family
        for (i, j, a, bb, cop) in edges:
            if cop != want:
                continue
            for _ in range(per):
                s = 0.1 + 0.8 * rng.random()
                x, v = _aim(rng, V_[a] + s * (V_[bb] - V_[a]), n_[i] + n_[j])
                xs_.append(x), vs_.append(v)
        if xs_:
            add(key, np.array(xs_), np.array(vs_))
    xs_, vs_ = [], []
    used = np.unique(faces)
    for vi in used:
        inc = np.nonzero((faces == vi).any(axis=1))[0]
        for _ in range(max(3, -(-120 // used.shape[0]))):
            x, v = _aim(rng, V_[vi], n_[inc].sum(axis=0) if np.linalg.norm(n_[inc].sum(axis=0)) > 1e-6 else n_[inc[0]])
            xs_.append(x), vs_.append(v)
    add('vertex', np.array(xs_), np.array(vs_))
    if planetie:
        # two planes tied for the smallest t, bit for bit: a seeded search among many edge-aimed rays, on the planes alone
        E = np.array([(i, j, a, bb) for (i, j, a, bb, cop) in edges if not cop])
        pick = E[rng.integers(0, E.shape[0], 40000)]
        tgt = V_[pick[:, 2]] + (0.1 + 0.8 * rng.random((40000, 1))) * (V_[pick[:, 3]] - V_[pick[:, 2]])
        nrm = n_[pick[:, 0]] + n_[pick[:, 1]]
        nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
        side = rng.normal(size=(40000, 3))
        side -= nrm * np.sum(side * nrm, axis=1, keepdims=True)
        h = 0.5 + 2.5 * rng.random((40000, 1))
        xs_ = tgt - nrm * h + 0.3 * h * rng.random((40000, 1)) * side / np.linalg.norm(side, axis=1, keepdims=True)
        vs_ = (tgt - xs_) / h
        tp = np.sort(plane_times(g, xs_, vs_)[0], axis=1)
        tie = np.nonzero(np.isfinite(tp[:, 0]) & (tp[:, 0] == tp[:, 1]))[0][:300]
        add('planetie', xs_[tie], vs_[tie])
    return np.concatenate(X), np.concatenate(V), fam, rng


LDS_SEEDS = {'box200ttp': 5, 'cyl': 6, 'corrugated': 7, 'castle': 8}


def lds_families(name):
    """Ray families on a small mesh (tables in LDS): {family: index array}, x, v, and the all-faces reference."""
    def make():
        g = lds_mesh(name)
        x, v, fam, _ = ray_families(g, LDS_SEEDS[name], 3000 if name in NONCONVEX_ARGS else 600, name in NONCONVEX_ARGS)
        return dict(x=x, v=v, fam=fam, ref=all_faces_cast(g, x, v))
    return cached(('lds_fam', name), make)


# ------------------------------------------------------------- meshes cast through the face tree
# More than 256 faces (NK_LDS_FACES): the tables stay in global memory and every cast walks the face tree.  The smallest meshes
# that reach every part of it: wire72 a tree of several levels over 288 faces with fan caps; star adds diagonal slivers and a
# non-convex section; longwire has side triangles of 13 A x 60 000 A, every one split into several references, and coordinates
# up to 6e4, where a float's ulp is 0.004 A.
TREE_BOUNDS = ['--bound_pos', 'relative', '0.5', '0.5', '0', '0.5', '0.5', '1', '--bound_cond', 'T', 'T', 'R',
               '--bound_values', '302', '298', '5']
TREE_ARGS = {
    'wire72': ['--geometry', 'cylinder', '--dimensions', '500', '100', '72', '--subvolumes', 'slice', '10', '2'],
    'star': ['--geometry', 'star', '--dimensions', '600', '200', '90', '72', '--subvolumes', 'slice', '4', '2'],
    'longwire': ['--geometry', 'cylinder', '--dimensions', '60000', '150', '72', '--subvolumes', 'slice', '10', '2'],
}
TREE_SEED = 6
TREE_NGEN = 600
SPEEDS = (1e-3, 1.0, 40.0, 1e4)
TINY = (0.0, 4.9e-324, 1e-310, 1e-40, 1e-25, 1e-12, 1e-6)


def tree_case(name):
    """case_from_args of a tree-sized mesh: ['mesh'] the tables, ['geo'].mesh the package's Mesh."""
    return cached(('tree_case', name), lambda: case_from_args(TREE_ARGS[name] + TREE_BOUNDS + COMMON_ARGS))


def tree_mesh(name):
    return tree_case(name)['mesh']


def side_faces(g):
    """Faces of the facets that are no end cap (caps: facet normal along the wire's axis z)."""
    nz = np.abs(np.asarray(g['facets_normal'], dtype=float)[:, 2])
    return np.nonzero(nz[np.asarray(g['face_facets'], dtype=int)] < 0.5)[0]


def cap_facets(g):
    """The two end caps: facets whose normal is +-e_z."""
    return [int(c) for c in np.nonzero(np.abs(np.asarray(g['facets_normal'], dtype=float)[:, 2]) == 1.0)[0]]


def _sliver_rays(g, rng):
    """Hits spread along the whole length of long side faces: towards points at fractions 2^-k, 1 - 2^-k and random ones of a
    face's longest edge -- on the edge itself (the diagonal it shares with its coplanar neighbour) and moved into the face --
    and rays nearly parallel to the axis that travel thousands of angstrom before they hit."""
    V_, faces = np.asarray(g['vertices'], dtype=float), np.asarray(g['faces'], dtype=int)
    n_ = np.asarray(g['face_normals'], dtype=float)
    X, V = [], []
    side = side_faces(g)
    for f in rng.choice(side, size=min(48, side.shape[0]), replace=False):
        P = V_[faces[f]]
        e = int(np.argmax([np.linalg.norm(P[(k + 1) % 3] - P[k]) for k in range(3)]))
        a, b, c = P[e], P[(e + 1) % 3], P[(e + 2) % 3]
        fr = [2.0 ** -k for k in range(1, 7)] + [1.0 - 2.0 ** -k for k in range(2, 7)] + list(rng.random(5))
        for i, s in enumerate(fr):
            tgt = a + s * (b - a)
            if i % 2:
                tgt = tgt + (0.05 + 0.6 * rng.random()) * (c - tgt)
            x, v = _aim(rng, tgt, n_[f])
            X.append(x), V.append(v)
    x0 = sample_inside(g, 7 * 24, rng)
    for i in range(x0.shape[0]):
        q = 1.0 - 10.0 ** -(3 + i % 7)                              # |v_z| / |v|
        phi = 2.0 * np.pi * rng.random()
        s = np.sqrt((1.0 - q) * (1.0 + q))
        X.append(x0[i]), V.append(40.0 * np.array([s * np.cos(phi), s * np.sin(phi), q if (i // 7) % 2 else -q]))
    return np.array(X), np.array(V)


def _tiny_rays(g, rng):
    """One component +-40, each of the others from +-TINY: every pair of values and signs once per axis and direction."""
    vals = [sg * t for t in TINY for sg in (1.0, -1.0)]
    V = []
    for a in range(3):
        for big in (40.0, -40.0):
            for p in vals:
                for q in vals:
                    v = np.array([p, q, q])
                    v[(a + 1) % 3], v[(a + 2) % 3], v[a] = p, q, big
                    V.append(v)
    V = np.array(V)
    return sample_inside(g, V.shape[0], rng), V


def _far_rays(g, rng, n=480):
    """Starts 1e3 .. 1e6 A from the body (where a float's ulp reaches 0.06 A: the |x| term of the slab test's widening), flying at
    |v| = 40 towards interior points, points of shared edges and vertices: near-ties at the end of a long flight, where the float
    tmax is all that stands between a worse hit found first and the better one."""
    V_, faces = np.asarray(g['vertices'], dtype=float), np.asarray(g['faces'], dtype=int)
    edges = _shared_edges(g)
    m = n // 3
    e = [edges[i] for i in rng.integers(0, len(edges), m)]
    s = 0.1 + 0.8 * rng.random((m, 1))
    on_edge = np.array([V_[a] for (_, _, a, _, _) in e]) + s * np.array([V_[b] - V_[a] for (_, _, a, b, _) in e])
    tgt = np.concatenate([sample_inside(g, n - 2 * m, rng), on_edge, V_[rng.choice(np.unique(faces), m)]])
    u = rng.normal(size=(n, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    dist = 10.0 ** (3.0 + 3.0 * rng.random((n, 1)))
    x = tgt + dist * u
    return x, (tgt - x) * (40.0 / dist)


def subtiny_rays(g, seed=TREE_SEED):
    """20 rays whose every component lies below 1e-30 in magnitude, in unequal ratio (1 : 3 : 0 and the like): all their 1 / v
    clamp to the same NK_RAY_BIG.  Outside the cast's stated domain (largest |v_a| >= 1e-25, nk_device.h); kept for probes."""
    rng = np.random.default_rng(seed + 1000)
    V = []
    for i in range(20):
        v = np.array([1.0, 3.0, 0.0, 1.0, -7.0, 2.0][i % 4:i % 4 + 3]) * 10.0 ** -(31 + i % 6)
        V.append(np.roll(v, i % 3) * (1.0 if i % 2 else -1.0))
    return sample_inside(g, 20, rng), np.array(V)


def tree_families(name):
    """ray_families on a tree-sized mesh plus the families of the tree's own filters: `speed` (|v| over seven orders of magnitude:
    tmax), `tiny` (components that are zero, denormal or so small that (float)(1 / v) overflows: the NK_RAY_BIG clamp), on
    longwire `sliver`, and `far` (starts up to 1e6 A away: the widening's |x| term, near-ties after long flights).  {x, v, fam, ref} like lds_families.  (`boxwall` needs the boxes of the device's tree: boxwall_rays.)"""
    def make():
        g = tree_mesh(name)
        x, v, fam, rng = ray_families(g, TREE_SEED, TREE_NGEN, False)
        X, V = [x], [v]

        def add(key, xs, vs):
            start = sum(a.shape[0] for a in X)
            X.append(xs), V.append(vs)
            fam[key] = np.arange(start, start + xs.shape[0])
        gi = fam['generic']
        d = v[gi] / np.linalg.norm(v[gi], axis=1, keepdims=True)
        add('speed', x[gi], d * np.array(SPEEDS)[np.arange(gi.shape[0]) % len(SPEEDS), None])
        add('tiny', *_tiny_rays(g, rng))
        if name == 'longwire':
            add('sliver', *_sliver_rays(g, rng))
        add('far', *_far_rays(g, rng))
        x, v = np.concatenate(X), np.concatenate(V)
        return dict(x=x, v=v, fam=fam, ref=all_faces_cast(g, x, v))
    return cached(('tree_fam', name), make)


def decided(ref):
    """Where the facet must be the reference's own rather than any member of the admissible set: one admissible facet, an exact
    tie between faces (then the lowest face index), or a miss.  Returns (decided, exact_tie)."""
    one = np.array([len(a) == 1 for a in ref['adm']])
    exact_tie = (ref['T'] == ref['tc'][:, None]).sum(axis=1) > 1
    return one | exact_tie | ~ref['hit'], exact_tie & ref['hit']


def boxwall_rays(g, info, seed=TREE_SEED, nboxes=40):
    """Rays at the walls of the tree's own boxes (Engine.tree_info(boxes=True)): about `nboxes` boxes over all levels, leaf face
    boxes included.  Per wall: two rays INSIDE the wall plane (the coordinate equals the wall's float exactly, v_a = +0.0 and
    -0.0, the rest random) and two that start on the wall and fly perpendicular to it, either way; per corner rays through it along
    (+-1, +-1, +-1) 2^k.  The starts spread over the box and a margin around it: some lie in the solid, some outside."""
    rng = np.random.default_rng(seed + 77)
    boxes = []
    per = max(2, nboxes // (len(info['family_boxes']) + 1))
    for lv in list(info['family_boxes']) + [info['leaf_boxes'].reshape(-1, 6)]:
        real = lv[lv[:, 0] <= lv[:, 3]].astype(np.float64)
        boxes += list(real[rng.choice(real.shape[0], size=min(per, real.shape[0]), replace=False)])
    X, V = [], []
    for B in boxes:
        lo, hi = B[:3], B[3:]
        ext = hi - lo
        for a in range(3):
            for wall in (lo[a], hi[a]):
                for z in (0.0, -0.0):
                    x = lo - 0.2 * ext + 1.4 * ext * rng.random(3)
                    v = rng.normal(size=3) * 40.0
                    x[a], v[a] = wall, z
                    X.append(x), V.append(v)
                for sg in (40.0, -40.0):
                    x = lo + ext * rng.random(3)
                    x[a] = wall
                    v = np.zeros(3)
                    v[a] = sg
                    X.append(x), V.append(v)
        for c in CORNERS:
            corner = np.array([hi[k] if c[k] else lo[k] for k in range(3)])
            for k in (-2, 5):
                d = rng.choice([-1.0, 1.0], size=3)
                X.append(corner - 2.0 * d), V.append(d * 2.0 ** k)
    x, v = np.array(X), np.array(V)
    return dict(x=x, v=v, nboxes=len(boxes), ref=all_faces_cast(g, x, v))


# the facet skip (nk_tree_skip, nk_device.h) restated
def facet_skip_tables(g):
    """Per facet (dn, dk) as nk_set_mesh forms them: the largest component of n_face - n_facet and the largest
    |n_face . centroid + k_face| over the facet's faces; dn = 1e300 ("never") for facets of fewer than 16 faces."""
    n_, k_ = np.asarray(g['face_normals'], dtype=float), np.asarray(g['face_k'], dtype=float)
    ff = np.asarray(g['face_facets'], dtype=int)
    fn, fc = np.asarray(g['facets_normal'], dtype=float), np.asarray(g['facet_centroid'], dtype=float)
    Fc = fn.shape[0]
    dn, dk = np.zeros(Fc), np.zeros(Fc)
    np.maximum.at(dn, ff, np.abs(n_ - fn[ff]).max(axis=1))
    c = fc[ff]
    np.maximum.at(dk, ff, np.abs(((n_[:, 0] * c[:, 0] + n_[:, 1] * c[:, 1]) + n_[:, 2] * c[:, 2]) + k_))
    dn[np.bincount(ff, minlength=Fc) < 16] = 1e300
    return dn, dk


def tree_skip_rule(g, from_facet, x, v, tol=TOL):
    """nk_tree_skip: skip where (dist + dn r + dk) 1.000001 + 1e-300 < tol / 2 (|v . n| - dn |v|_1).  Returns (skip, lhs, rhs);
    names outside [0, Fc) never skip (lhs = inf)."""
    fn, fc = np.asarray(g['facets_normal'], dtype=float), np.asarray(g['facet_centroid'], dtype=float)
    dn, dk = facet_skip_tables(g)
    ff = np.asarray(from_facet, dtype=int)
    ok = (ff >= 0) & (ff < fn.shape[0])
    f = np.where(ok, ff, 0)
    r_ = x - fc[f]
    n = fn[f]
    with np.errstate(all='ignore'):
        dist = np.abs((r_[:, 0] * n[:, 0] + r_[:, 1] * n[:, 1]) + r_[:, 2] * n[:, 2])
        r1, vv = np.abs(r_).sum(axis=1), np.abs(v).sum(axis=1)
        vn = np.abs((v[:, 0] * n[:, 0] + v[:, 1] * n[:, 1]) + v[:, 2] * n[:, 2])
        lhs = np.where(ok, (dist + dn[f] * r1 + dk[f]) * 1.000001 + 1e-300, np.inf)
        rhs = 0.5 * tol * (vn - dn[f] * vv)
    return lhs < rhs, lhs, rhs


SKIP_C = (0.125, 0.499, 0.501, 1.0, 4.0, 1e4)
SKIP_GRAZE = (0.0, 1e-9, 1e-6, 1e-3)


def skip_families(name):
    """Rays for the facet skip on a mesh with fan caps: {x, v, from_facet, fam}.
    (a) 1500 starts on each cap (Mesh.sample_surface), random inward directions; (b) starts of (a) moved along the normal by
    +-c tol |v.n|, c in SKIP_C: the cap's own t straddles tol / 2 and tol; (c) grazing and outward rays, |v.n| / |v| in SKIP_GRAZE
    of either sign; (d) starts on the cap's rim vertices and rim edges; (e) starts of (a) under wrong names: the other cap, a side
    facet, -1 and Fc."""
    def make():
        ct = tree_case(name)
        g, mesh = ct['mesh'], ct['geo'].mesh
        rng = np.random.default_rng(TREE_SEED + 200)
        fn = np.asarray(g['facets_normal'], dtype=float)
        V_, faces, ff = np.asarray(g['vertices'], dtype=float), np.asarray(g['faces'], dtype=int), np.asarray(g['face_facets'], dtype=int)
        caps = cap_facets(g)
        assert len(caps) == 2
        side = int(np.nonzero(np.abs(fn[:, 2]) < 0.5)[0][0])
        X, V, FF, fam = [], [], [], {}

        def add(key, xs, vs, names):
            start = sum(a.shape[0] for a in X)
            X.append(xs), V.append(vs), FF.append(np.broadcast_to(np.asarray(names, dtype=np.int32), (xs.shape[0],)).copy())
            fam[key] = np.concatenate([fam.get(key, np.zeros(0, dtype=int)), np.arange(start, start + xs.shape[0])])

        def inward(n, m):
            v = rng.normal(size=(m, 3)) * 40.0
            vn = v @ n
            return v - np.outer(vn + np.abs(vn), n)                  # v.n -> -|v.n|
        for ci, cap in enumerate(caps):
            n = fn[cap]
            xa = mesh.sample_surface(1500, facets=[cap], rng=rng)
            va = inward(n, 1500)
            add('a', xa, va, cap)
            xb, vb = xa[:100], va[:100]
            for c in SKIP_C:
                for sg in (1.0, -1.0):
                    add('b', xb + np.outer(sg * c * TOL * np.abs(vb @ n), n), vb, cap)
            t1 = np.cross(n, [1.0, 0.0, 0.0])
            t2 = np.cross(n, t1)
            for q in SKIP_GRAZE:
                for sg in (1.0, -1.0):
                    phi = 2.0 * np.pi * rng.random(50)
                    tang = np.outer(np.cos(phi), t1) + np.outer(np.sin(phi), t2)
                    add('c', xa[200:250], 40.0 * (np.sqrt((1.0 - q) * (1.0 + q)) * tang + sg * q * n), cap)
            add('c', xa[250:400], -inward(n, 150), cap)                     # outward
            cf = faces[ff == cap]
            vid, cnt = np.unique(cf, return_counts=True)
            rim = vid[cnt < cnt.max()] if cnt.max() > 2 else vid         # (a fan's centre belongs to every face of the cap)
            add('d', V_[rim], inward(n, rim.shape[0]), cap)
            re = np.array([sorted(e) for tri in cf for e in ((tri[0], tri[1]), (tri[1], tri[2]), (tri[2], tri[0]))
                           if e[0] in rim and e[1] in rim])
            s = rng.random((re.shape[0], 1))
            add('d', V_[re[:, 0]] + s * (V_[re[:, 1]] - V_[re[:, 0]]), inward(n, re.shape[0]), cap)
            for wrong in (caps[1 - ci], side, -1, fn.shape[0]):
                add('e', xa[:200], va[:200], wrong)
        return dict(x=np.concatenate(X), v=np.concatenate(V), from_facet=np.concatenate(FF), fam=fam, caps=caps)
    return cached(('skip_fam', name), make)


# ------------------------------------------------------------------------------ slice lookups
S_MAX_TAP = 160       # nk_set_subvolumes takes S <= 512, and the taps' LDS tables fit the default 64 KB up to S = 180


def slice_sets():
    """{name: dict(centers [S, 3], axis, T_sv [S])}: the goldens' slices and hand-made ones by the reference's formula
    np.linspace(0, 1 - 1/n, n) + 1/(2n) times the length."""
    def make():
        out = {}
        for name in ('box200', 'box5000', 'cyl'):
            g = sub(golden('mesh'), name)
            out[name] = dict(centers=np.asarray(g['subvol_center'], dtype=float), axis=int(g['slice_axis']),
                             bounds=np.asarray(g['bounds'], dtype=float))
        L = np.array([200.0, 123.4567, 350.0])
        for S in (1, 2, 7, S_MAX_TAP):
            for axis in range(3):
                c = np.tile(0.5 * L, (S, 1))
                c[:, axis] = (np.linspace(0, 1 - 1 / S, S) + 1 / (2 * S)) * L[axis]
                out['hand_S%d_ax%d' % (S, axis)] = dict(centers=c, axis=axis, bounds=np.array([np.zeros(3), L]))
        for k, (name, d) in enumerate(sorted(out.items())):
            S = d['centers'].shape[0]
            # a gentle profile: the linear rule's product slope (xa - c) stays small against T even 1000 A outside the box
            d['T_sv'] = 299.0 + 2.0 * (np.arange(S) + 0.37) / S + 1e-4 * np.random.default_rng(k).random(S)
            assert np.unique(d['T_sv']).shape[0] == S
        return out
    return cached('slice_sets', make)


def slice_points(name):
    """Points at every slice edge (the double c[i+1]/2 + c[i]/2) and every centre: 0, +-1, +-2, +-5, +-50 ulps, +-1e-12 A,
    +-0.5e-9 and +-2e-9 slice widths; one ulp, 1 A and 1000 A outside either end; random off-axis coordinates.
    Returns x [n, 3], and |offset| [n] in angstrom from the base point (inf for the outside points)."""
    def make():
        d = slice_sets()[name]
        c, a = d['centers'][:, d['axis']], d['axis']
        S = c.shape[0]
        rng = np.random.default_rng(S * 7 + a)
        wdt = (c[1] - c[0]) if S > 1 else (d['bounds'][1, a] - d['bounds'][0, a])
        base = np.concatenate([c[1:] / 2.0 + c[:-1] / 2.0, c])
        xa, off = [], []
        for k in (0, 1, -1, 2, -2, 5, -5, 50, -50):
            s = ulp_shift(base, k)
            xa.append(s), off.append(np.abs(s - base))
        for dlt in (1e-12, -1e-12, 0.5e-9 * wdt, -0.5e-9 * wdt, 2e-9 * wdt, -2e-9 * wdt):
            xa.append(base + dlt), off.append(np.abs((base + dlt) - base))
        lo_end, hi_end = c[0] - wdt / 2.0, c[-1] + wdt / 2.0
        ends = np.array([np.nextafter(lo_end, -np.inf), lo_end - 1.0, lo_end - 1000.0, np.nextafter(hi_end, np.inf), hi_end + 1.0,
                         hi_end + 1000.0, lo_end, hi_end])
        xa.append(ends), off.append(np.full(ends.shape[0], np.inf))
        xa, off = np.concatenate(xa), np.concatenate(off)
        x = d['bounds'][0] + rng.random((xa.shape[0], 3)) * (d['bounds'][1] - d['bounds'][0])
        x[:, a] = xa
        return x, off
    return cached(('slice_points', name), make)


def exact_nearest_1d(c, xa):
    """Index of the centre nearest to xa along the axis, exactly; the lowest index on ties."""
    cf = [Fr(float(v)) for v in c]
    j = np.searchsorted(c, xa)
    out = np.zeros(xa.shape[0], dtype=np.int32)
    S = len(cf)
    for i in range(xa.shape[0]):
        q = Fr(float(xa[i]))
        cand = range(max(0, j[i] - 2), min(S, j[i] + 2))
        out[i] = min(cand, key=lambda s: (abs(q - cf[s]), s))
    return out


def oracle_band(centers, x, idx):
    """Where the oracle's rounded 3-D squared distances may name another slice than the exact rule: the exact gap
    |d1^2 - d2^2| between the nearest centre (idx) and the nearest of its neighbours is below 8 u max(d1^2, d2^2), the rounding
    of a three-term squared distance.  Returns the boolean array `small`."""
    S = centers.shape[0]
    cf = [[Fr(float(v)) for v in row] for row in centers]
    small = np.zeros(x.shape[0], dtype=bool)
    if S == 1:
        return small
    for i in range(x.shape[0]):
        q = [Fr(float(v)) for v in x[i]]
        d2 = {}
        for s in (idx[i] - 1, idx[i], idx[i] + 1):
            if 0 <= s < S:
                d2[s] = sum((q[k] - cf[s][k]) ** 2 for k in range(3))
        d1 = d2.pop(int(idx[i]))
        dn = min(d2.values())
        small[i] = abs(d1 - dn) < 8 * U * max(d1, dn)
    return small


def slice_reference(name):
    """(exact nearest centre of every point of slice_points(name), whether it lies in the oracle's rounding band)."""
    def make():
        d = slice_sets()[name]
        x, _ = slice_points(name)
        idx = exact_nearest_1d(d['centers'][:, d['axis']], x[:, d['axis']])
        return idx, oracle_band(d['centers'], x, idx)
    return cached(('slice_reference', name), make)


def nearest_bounds_rule(c, xa):
    """interp1d(kind='nearest'): bounds b[i] = c[i+1]/2 + c[i]/2 in double, idx = #(b < xa)."""
    b = c[1:] / 2.0 + c[:-1] / 2.0
    return np.searchsorted(b, xa, side='left').astype(np.int32)


def exact_linear_T(c, T, xa):
    """interp1d(kind='linear', fill_value='extrapolate') as the oracle states it: idx = searchsorted(c, xa, 'left') clipped to
    [1, S-1], slope = (T[idx] - T[idx-1]) / (c[idx] - c[idx-1]) in double, and then slope (xa - c[idx-1]) + T[idx-1] EXACTLY."""
    S = c.shape[0]
    idx = np.clip(np.searchsorted(c, xa, side='left'), 1, S - 1)
    slope = (T[idx] - T[idx - 1]) / (c[idx] - c[idx - 1])
    return [Fr(float(slope[i])) * (Fr(float(xa[i])) - Fr(float(c[idx[i] - 1]))) + Fr(float(T[idx[i] - 1])) for i in range(xa.shape[0])], idx


# ------------------------------------------------------------------------------ grid subvolumes
def grid_case():
    """4 x 4 x 2 centres on the 200 A box (all doubles exact); points exactly on bisector planes, edges and corners of the
    cells (exact ties), the same moved by a few ulps, and random points."""
    def make():
        cx, cz = np.array([25.0, 75.0, 125.0, 175.0]), np.array([50.0, 150.0])
        cen = np.array([[x, y, z] for x in cx for y in cx for z in cz])
        rng = np.random.default_rng(31)
        bx, bz = [50.0, 100.0, 150.0], [100.0]
        P = []
        for _ in range(40):
            p = rng.random(3) * 200.0
            on = rng.integers(1, 8)                                  # which coordinates sit on a bisector (bit mask)
            for a in range(3):
                if on >> a & 1:
                    p[a] = rng.choice(bx if a < 2 else bz)
            P.append(p)
        for x in bx:
            for y in bx:
                P.append([x, y, 100.0])                              # corners of the cells: eight-fold ties
        tie = np.array(P)
        moved = tie.copy()
        for i in range(moved.shape[0]):
            for a in range(3):
                moved[i, a] = ulp_shift(moved[i, a], int(rng.integers(-3, 4)))
        return dict(centers=cen, tie=tie, moved=moved, rand=rng.random((2000, 3)) * 200.0)
    return cached('grid', make)


def exact_nearest_3d(centers, x):
    """Per point the sorted list of the centres at the exact smallest distance."""
    cf = [[Fr(float(v)) for v in row] for row in centers]
    out = []
    for p in x:
        q = [Fr(float(v)) for v in p]
        d2 = [sum((q[k] - c[k]) ** 2 for k in range(3)) for c in cf]
        m = min(d2)
        out.append([s for s, v in enumerate(d2) if v == m])
    return out


# ------------------------------------------------------------------------------ material tables
def tau_window(g, T_lo, T_hi):
    """The packed window (g0, g2] that nk_update_tau_window chooses for subvolume temperatures in [T_lo, T_hi]: row0 and the
    three grid values; None when the table has fewer than three rows."""
    NT = g.shape[0]
    if NT < 3:
        return None
    Tm = 0.5 * (T_lo + T_hi)
    i = max(int(np.searchsorted(g, Tm, side='left')) - 1, 0)
    row0 = i if (i + 1 < NT and T_hi - g[min(i + 1, NT - 1)] > g[i] - T_lo) else i - 1
    row0 = max(min(row0, NT - 3), 0)
    return row0, g[row0:row0 + 3].copy()


TAU_SETTINGS = {'all300': (300.0, 300.0), 'lowest': (200.0, 200.0), 'highest': (400.0, 400.0), 'wide': (250.0, 350.0),
                'node': (319.9, 320.1)}


def lifetime_temperatures(g, window, seed):
    """Every grid node and window value +-1 ulp, midpoints, 2000 random T in the table; and the inputs that give NaN."""
    rng = np.random.default_rng(seed)
    nodes = np.concatenate([g, window[1]]) if window is not None else g
    T = np.concatenate([ulp_shift(nodes, k) for k in (0, 1, -1)] + [0.5 * (g[1:] + g[:-1]), g[0] + rng.random(2000) * (g[-1] - g[0])])
    T = T[(T >= g[0]) & (T <= g[-1])]
    bad = np.array([np.nextafter(g[0], -np.inf), np.nextafter(g[-1], np.inf), np.inf, -np.inf, np.nan])
    return T, bad


def exact_lifetime(g, tau, T, mode):
    """RegularGridInterpolator along T at a grid point of (q, j): i = searchsorted(g, T, 'left') - 1 clipped to [0, NT-2],
    y = (T - g[i]) / (g[i+1] - g[i]), tau[i] (1 - y) + tau[i+1] y, exactly."""
    NT = g.shape[0]
    tau = tau.reshape(NT, -1)
    i = np.clip(np.searchsorted(g, T, side='left') - 1, 0, NT - 2)
    out = []
    for n in range(T.shape[0]):
        y = (Fr(float(T[n])) - Fr(float(g[i[n]]))) / (Fr(float(g[i[n] + 1])) - Fr(float(g[i[n]])))
        out.append(Fr(float(tau[i[n], mode[n]])) * (1 - y) + Fr(float(tau[i[n] + 1, mode[n]])) * y)
    return out


def cut_tables(tb, rows):
    """A copy of the material tables with only the given rows of the temperature grid (NT = len(rows))."""
    out = dict(tb)
    out['T_grid'] = np.ascontiguousarray(np.asarray(tb['T_grid'], dtype=float)[rows])
    out['lifetime'] = np.ascontiguousarray(np.asarray(tb['lifetime'], dtype=float)[rows])
    return out


def table_points(xs, seed):
    """Every node +-1 ulp, random interior values; and one ulp and far outside either end."""
    rng = np.random.default_rng(seed)
    inner = np.concatenate([ulp_shift(xs, 1)[:-1], ulp_shift(xs, -1)[1:], xs[0] + rng.random(2000) * (xs[-1] - xs[0])])
    span = xs[-1] - xs[0]
    outside = np.array([np.nextafter(xs[0], -np.inf), xs[0] - span, np.nextafter(xs[-1], np.inf), xs[-1] + 10 * span])
    return xs.copy(), inner, outside


def exact_interp(xs, ys, x):
    """Exact linear interpolation of the table's doubles (bracket of scipy interp1d: searchsorted 'left' clipped to [1, n-1])."""
    n = xs.shape[0]
    idx = np.clip(np.searchsorted(xs, x, side='left'), 1, n - 1)
    out = []
    for i in range(x.shape[0]):
        x0, x1, y0, y1 = (Fr(float(v)) for v in (xs[idx[i] - 1], xs[idx[i]], ys[idx[i] - 1], ys[idx[i]]))
        out.append(y0 + (y1 - y0) * (Fr(float(x[i])) - x0) / (x1 - x0))
    return out
