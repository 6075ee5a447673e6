"""Free-path sampling on the CPU: the rule of nk_free_paths (DESIGN.md "Free-path sampling") restated in NumPy, vectorised over
the rays, with the oracle's ray cast (nko_find_boundary) and random numbers (nko_uniform2) and NumPy's expm1 / exp.  What the
GPU tests hold the kernel against, and the cases they share.  Test infrastructure: nothing under nanokappa_amd/ knows of it."""
import ctypes as C
import os
import sys

import numpy as np

from util import case_tables, case_from_args

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'oracle'))
import nk_oracle as O  # noqa: E402

TAG_FREE = 0x50000            # NK_TAG_FREE (nanokappa_amd/csrc/nk_freepath.h; the draws are made in nk_flight.h)
W_MIN = 2.0 ** -40
MAX_SEGMENTS = 65536
_CACHE = {}


def cached(key, make):
    """Computed once per process and shared by the tests; callers must not modify the result."""
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def uniform2(seed, pid, step, tag):
    a, b = C.c_double(), C.c_double()
    O.lib().nko_uniform2(C.c_uint64(int(seed)), C.c_uint64(int(pid)), C.c_uint32(int(step)), C.c_uint32(int(tag)), C.byref(a), C.byref(b))
    return a.value, b.value


def find_boundary(mesh, x, v):
    n = x.shape[0]
    x, v = np.ascontiguousarray(x, dtype=np.float64), np.ascontiguousarray(v, dtype=np.float64)
    xc, tc, fc = np.zeros((n, 3)), np.zeros(n), np.zeros(n, dtype=np.int32)
    P = lambda a, t=O.c_dp: a.ctypes.data_as(t)
    O.lib().nko_find_boundary(C.byref(mesh), C.c_int64(n), P(x), P(v), P(xc), P(tc), P(fc, O.c_ip))
    return tc, fc


def fma(a, b, c):
    """a * b + c with one rounding (but for rare double roundings of the last step): the product's error by Dekker's split, the
    sum's by Knuth's two-sum.  The kernel forms its hit points with a fused multiply-add."""
    a, b, c = np.broadcast_arrays(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), np.asarray(c, dtype=np.float64))
    p = a * b
    k = 134217729.0
    ah = k * a - (k * a - a)
    al = a - ah
    bh = k * b - (k * b - b)
    bl = b - bh
    e = ((ah * bh - p) + ah * bl + al * bh) + al * bl
    s = p + c
    bb = s - p
    t = (p - (s - bb)) + (c - bb)
    return s + (t + e)


def simplex_cdf(g):
    """nk_set_mesh's cumulative volume fractions of the simplices."""
    vol = np.asarray(g['simplices_volumes'], dtype=np.float64)
    tot = 0.0
    for x in vol:
        tot += x
    sc, acc = np.zeros(vol.shape[0]), 0.0
    for i, x in enumerate(vol):
        acc += x / tot
        sc[i] = acc
    return sc / sc[-1]


def start_points(g, modes, n, seed):
    """The device sampler's draws: for ray (mode, sample), id (mode << 32) | sample, three uniform pairs with step 0 and tags
    TAG_FREE + 0..2 -> simplex by volume (searchsorted right), barycentric weights -log(u) / sum.  [L, n, 3]."""
    sc = simplex_cdf(g)
    pts = np.asarray(g['simplices_points'], dtype=np.float64)[np.asarray(g['simplices'], dtype=int)]      # [nS, 4, 3]
    out = np.zeros((len(modes), n, 3))
    for li, m in enumerate(modes):
        for s in range(n):
            rid = (int(m) << 32) | s
            u0, u1 = uniform2(seed, rid, 0, TAG_FREE + 0)
            u2, u3 = uniform2(seed, rid, 0, TAG_FREE + 1)
            u4, _ = uniform2(seed, rid, 0, TAG_FREE + 2)
            sx = min(int(np.searchsorted(sc, u0, side='right')), sc.shape[0] - 1)
            a = -np.log(np.array([u1, u2, u3, u4]))
            asum = ((a[0] + a[1]) + a[2]) + a[3]
            x = np.zeros(3)
            for q in range(4):
                x = x + (a[q] / asum) * pts[sx, q]
            out[li, s] = x
    return out


def facet_tables(g, rough=None):
    bc = np.asarray(g['bound_cond'])
    if bc.dtype.kind in 'US':
        bc = np.array([ord(str(c)[0]) for c in bc])
    bc = bc.astype(np.int64)
    Fc = bc.shape[0]
    cen = np.asarray(g['facet_centroid'], dtype=np.float64)
    partner = -np.ones(Fc, dtype=np.int64)
    for a, b in np.asarray(g.get('connected_facets', np.zeros((0, 2))), dtype=int).reshape(-1, 2):
        partner[a], partner[b] = b, a
    trans = np.where(partner[:, None] >= 0, cen[np.maximum(partner, 0)] - cen, 0.0)
    ridx = -np.ones(Fc, dtype=np.int64)
    if rough is not None:
        for i, f in enumerate(np.asarray(rough['facets'], dtype=int)):
            ridx[f] = i
    return bc, trans, ridx


def restate(g, group_vel, tau, modes, n, x0=None, seed=0, max_segments=MAX_SEGMENTS, w_min=W_MIN, rough=None, J=None, fused=True):
    """The rule for the rays of `modes` x n.  g: mesh tables; group_vel [M, 3]; tau [M]; x0 [L, n, 3] or None (drawn);
    rough: dict facets, specularity, true_spec, spec_map [Fr, M], degen_j2 [M] or None.  fused: the hit point as one fused
    multiply-add (the kernel's) or as a product and a sum.  Returns per ray D [L, n, 3], T, segments (casts), end, x0, seq (a
    hash of the facets met, in order) and per mode the sums D, D2, T, hits, p_res, p_wall, w_left, p_int, plus casts, missed,
    capped."""
    mesh = O.make_mesh(g)
    vg = np.asarray(group_vel, dtype=np.float64).reshape(-1, 3)
    tau = np.asarray(tau, dtype=np.float64).ravel()
    M = vg.shape[0]
    modes = np.asarray(modes, dtype=np.int64).ravel()
    L = modes.shape[0]
    R = L * n
    bc, trans, ridx = facet_tables(g, rough)
    if x0 is None:
        x0 = start_points(g, modes, n, seed)
    x0 = np.array(x0, dtype=np.float64).reshape(R, 3)
    m0 = np.repeat(modes, n)
    rid = (m0.astype(np.uint64) << np.uint64(32)) | np.tile(np.arange(n, dtype=np.uint64), L)
    D, T = np.zeros((R, 3)), np.zeros(R)
    W, k, ncast = np.ones(R), np.zeros(R, dtype=np.int64), np.zeros(R, dtype=np.int64)
    end = np.zeros(R, dtype=np.int32)
    seq = np.zeros(R, dtype=np.uint64)
    hits, p_res, p_wall, w_left, p_int = (np.zeros(R) for _ in range(5))
    missed, capped = np.zeros(R, dtype=np.int64), np.zeros(R, dtype=np.int64)
    mode = m0.copy()
    x = x0.copy()
    # modes that do not fly or do not live take no cast
    still = (tau[m0] > 0) & (np.abs(vg[m0]).max(axis=1) > 0)
    T[~still] = np.where(tau[m0[~still]] > 0, tau[m0[~still]], 0.0)         # (the kernel's tau > 0 ? tau : 0: a NaN lifetime gives 0)
    p_int[~still] = 1.0
    act = np.nonzero(still)[0]
    while act.size:
        v, t = vg[mode[act]], tau[mode[act]]
        tc, fc = find_boundary(mesh, x[act], v)
        ncast[act] += 1
        miss = fc < 0
        if miss.any():
            i = act[miss]
            wt = W[i] * t[miss]
            D[i] += wt[:, None] * v[miss]
            T[i] += wt
            p_int[i] += W[i]
            missed[i] += 1
            end[i] = 3
        hit = ~miss
        i, v, t, tc, fc = act[hit], v[hit], t[hit], tc[hit], fc[hit].astype(np.int64)
        a = tc / t
        gg, e = -np.expm1(-a), np.exp(-a)
        wt = W[i] * t * gg
        D[i] += wt[:, None] * v
        T[i] += wt
        p_int[i] += W[i] * gg
        W[i] *= e
        k[i] += 1
        hits[i] += W[i]
        seq[i] = seq[i] * np.uint64(1000003) + (fc + 2).astype(np.uint64)
        b = bc[fc]
        res = (b == ord('T')) | (b == ord('F'))
        p_res[i[res]] += W[i[res]]
        end[i[res]] = 1
        hp = fma(tc[:, None], v, x[i]) if fused else x[i] + tc[:, None] * v
        per = b == ord('P')
        x[i[per]] = hp[per] + trans[fc[per]]
        go = per.copy()
        ro = ~res & ~per
        if ro.any():
            for j in np.nonzero(ro)[0]:
                r = i[j]
                r0, r1 = uniform2(seed, rid[r], k[r], TAG_FREE + 3)
                f = ridx[fc[j]]
                out = int(rough['spec_map'][f, mode[r]]) if f >= 0 else -1
                spec = f >= 0 and bool(rough['true_spec'][f, mode[r]]) and r0 <= rough['specularity'][f, mode[r]] and 0 <= out < M
                if not spec:
                    p_wall[r] += W[r]
                    end[r] = 2
                    continue
                dj = rough.get('degen_j2')
                if dj is not None:
                    j2 = int(dj[out])
                    if -1 < j2 < J and r1 >= 0.5:
                        out = (out // J) * J + j2
                mode[r] = out
                x[r] = hp[j]
                if not tau[out] > 0:
                    p_int[r] += W[r]
                    end[r] = 0
                    continue
                go[j] = True
        i = i[go]
        low = W[i] < w_min
        w_left[i[low]] += W[i[low]]
        end[i[low]] = 0
        i = i[~low]
        cap = k[i] >= max_segments
        w_left[i[cap]] += W[i[cap]]
        capped[i[cap]] += 1
        end[i[cap]] = 4
        act = i[~cap]
    sh = (L, n)
    per_mode = lambda a: a.reshape(sh + a.shape[1:]).sum(axis=1)
    return dict(modes=modes.astype(np.int32), n=n, ray_D=D.reshape(L, n, 3), ray_T=T.reshape(sh), ray_segments=ncast.reshape(sh).astype(np.int32),
                ray_end=end.reshape(sh), ray_x0=x0.reshape(L, n, 3), ray_seq=seq.reshape(sh),
                D=per_mode(D), D2=per_mode(D * D), T=per_mode(T), hits=per_mode(hits), p_res=per_mode(p_res), p_wall=per_mode(p_wall),
                w_left=per_mode(w_left), p_int=per_mode(p_int),
                report=dict(rays=R, casts=int(ncast.sum()), missed=int(missed.sum()), capped=int(capped.sum())))


# ------------------------------------------------------------------------------------------- cases
T_CASE = 300.0


def case(name):
    """A case_tables-shaped dict by name: 'ttp' (box 200^3, T T P), 'ttrrp' ('velocity' tables), 'ttrrp_k' ('k' tables with
    degen_j2), 'corrugated' (non-convex wire, tables in LDS), 'wire72' (288 faces: tables in global memory)."""
    def make():
        if name == 'ttp':
            return case_tables('ttp')
        if name == 'ttrrp':
            return case_tables('ttrrp', 'velocity')
        if name == 'ttrrp_k':
            from nanokappa_amd import setup_tables as ST
            ct = dict(case_tables('ttrrp', 'k'))
            ph = ct['ph']
            Q, J = ph.omega.shape
            deg, idx = ST.find_degeneracies(ph)
            dj = -np.ones((Q, J), dtype=np.int32)
            has = idx.astype(int) > -1
            dj[has] = deg[idx.astype(int)[has], 2]
            ct['rough'] = dict(ct['rough'], degen_j2=dj.ravel())
            return ct
        from edge_cases import NONCONVEX_ARGS, COMMON_ARGS
        if name == 'corrugated':
            return case_from_args(NONCONVEX_ARGS['corrugated'] + COMMON_ARGS)
        if name == 'wire72':
            argv = ['--geometry', 'cylinder', '--dimensions', '500', '100', '72', '--subvolumes', 'slice', '10', '2',
                    '--bound_pos', 'relative', '0.5', '0.5', '0', '0.5', '0.5', '1', '--bound_cond', 'T', 'T', 'R',
                    '--bound_values', '302', '298', '5']
            return case_from_args(argv + COMMON_ARGS)
        raise KeyError(name)
    return cached(('case', name), make)


def lifetimes(ct, T=T_CASE):
    from nanokappa_amd import free_path as FP
    return FP.lifetimes(ct['ph'], T)


def group_vel(ct):
    return np.asarray(ct['tables']['group_vel'], dtype=np.float64).reshape(-1, 3)


def active_modes(ct, T=T_CASE):
    from nanokappa_amd import free_path as FP
    return FP.default_modes(group_vel(ct), lifetimes(ct, T))


def uniform_points(ct, L, n, seed):
    """Start points uniform in the solid from NumPy's generator (the x0 a test hands to both sides): the box directly, any
    other mesh through the package's Mesh.sample_volume."""
    rng = np.random.default_rng(seed)
    if 'geo' in ct:
        return np.asarray(ct['geo'].mesh.sample_volume(L * n, rng), dtype=np.float64).reshape(L, n, 3)
    b = np.asarray(ct['mesh']['bounds'], dtype=np.float64)
    return b[0] + rng.random((L, n, 3)) * (b[1] - b[0])


def ttp_modes_200(ct):
    """200 modes of 'ttp': every fourth mode with v_x = 0 among the active ones, the rest spread evenly over the others."""
    act = active_modes(ct)
    v = group_vel(ct)
    zero = act[v[act, 0] == 0][::4]
    other = act[v[act, 0] != 0]
    rest = other[np.linspace(0, other.shape[0] - 1, 200 - min(zero.shape[0], 100)).astype(int)]
    return np.unique(np.concatenate([zero[:100], rest])).astype(np.int32)


def run_case(name, modes, n, seed, max_segments=MAX_SEGMENTS, x0_seed=None, fused=True, x0='numpy'):
    """The restatement on a named case (cached by all its arguments)."""
    modes = np.asarray(modes, dtype=np.int32)

    def make():
        ct = case(name)
        pts = uniform_points(ct, modes.shape[0], n, seed if x0_seed is None else x0_seed) if x0 == 'numpy' else None
        return restate(ct['mesh'], group_vel(ct), lifetimes(ct), modes, n, x0=pts, seed=seed, max_segments=max_segments,
                       rough=ct['rough'], J=ct['J'], fused=fused)
    return cached(('run', name, modes.tobytes(), n, seed, max_segments, x0_seed, fused, x0), make)


def spread_modes(ct, count):
    """`count` active modes spread evenly over the list."""
    act = active_modes(ct)
    return act[np.linspace(0, act.shape[0] - 1, count).astype(int)].astype(np.int32)


# The per-ray comparisons of the GPU tests (tests/test_gpu_free_path.py), and the inputs test_free_path_host.py checks them on:
# name -> case, modes, rays per mode, max_segments, seed (of the start points and of the reflections' draws)
PARITY = {
    # n = 100: the second pass of lanes is partly empty; 256 segments: the cap path runs (152 of the 4368 modes exceed them)
    'ttp': dict(case='ttp', modes=ttp_modes_200, n=100, max_segments=256, seed=21),
    'ttrrp': dict(case='ttrrp', modes=lambda ct: spread_modes(ct, 256), n=64, max_segments=MAX_SEGMENTS, seed=22),
    'ttrrp_k': dict(case='ttrrp_k', modes=lambda ct: spread_modes(ct, 256), n=64, max_segments=MAX_SEGMENTS, seed=23),
    'corrugated': dict(case='corrugated', modes=lambda ct: spread_modes(ct, 64), n=64, max_segments=MAX_SEGMENTS, seed=24),
    'wire72': dict(case='wire72', modes=lambda ct: spread_modes(ct, 48), n=64, max_segments=MAX_SEGMENTS, seed=25),
}
MAX_OTHER_SEQUENCE = 1e-3     # share of rays whose facet sequence may differ between two evaluations of the hit point


def parity_run(name, fused=True):
    p = PARITY[name]
    ct = case(p['case'])
    return run_case(p['case'], p['modes'](ct), p['n'], p['seed'], max_segments=p['max_segments'], fused=fused)


# ------------------------------------------------------------------------------------------- recorded results
# The three free-path calls on short lists that reach every branch of the flight (tests/test_gpu_free_flight.py holds the engine
# against tests/golden/free_flight_<name>.npz, which scripts/free_path_golden.py records): name -> case, active modes in the list,
# rays per mode, max_segments, seed.  Every list also holds a mode that takes no cast and its first mode a second time.
GOLDEN = {
    'ttp': dict(case='ttp', active=4, n=100, max_segments=8, seed=31),          # periodic walls; the rays end by the cap
    'ttrrp_k': dict(case='ttrrp_k', active=4, n=64, max_segments=0, seed=32),   # specular turns, degenerate partner, diffuse ends
    'wire72': dict(case='wire72', active=3, n=64, max_segments=0, seed=33),     # the face tree; five entries: a workgroup of one wave
}
GOLDEN_COLUMNS = np.array([0.25, 0.375, 0.5, 0.75, 1.0, 1.5, 2.0, 3.0, 4.0])    # nine: one more than the column tile
GOLDEN_GRID = (3, 2, 2)


def golden_inputs(name):
    """What the recorded calls of a case are made with: tau [M], modes [L], weight [L, 3], the grid (lo, h, n_cells) -- lo is moved
    into the solid by 0.3 cells, so some start points lie outside the grid and are clamped -- and, for 'ttrrp_k', a table of
    degenerate partners (the case's own names none for a mode that a reflection leads to)."""
    from nanokappa_amd import field as FD
    from test_free_map_host import case_weights
    p = GOLDEN[name]
    ct = case(p['case'])
    tau = np.array(lifetimes(ct), dtype=np.float64)
    v = group_vel(ct)
    act = spread_modes(ct, p['active'])
    b = np.asarray(ct['mesh']['bounds'], dtype=np.float64).reshape(2, 3)
    out = {}
    if name == 'ttp':
        # two modes that fly along the reservoirs and meet periodic walls alone: one ends by the cap, the other, with a lifetime of
        # a tenth of a crossing, by its weight
        along = active_modes(ct)
        along = along[v[along, 0] == 0]
        act = np.array([along[0], act[1], along[along.shape[0] // 2], act[2]])
        tau[act[2]] = (b[1] - b[0]).max() / (10.0 * np.abs(v[act[2]]).max())
    if name == 'ttrrp_k':
        # modes that a rough facet reflects specularly, as often as the tables allow, into another mode; every second mode gets
        # the next branch at its wave vector as its degenerate partner
        r, J = ct['rough'], ct['J']
        sp = np.where(np.asarray(r['true_spec']) & (np.asarray(r['spec_map']) >= 0), np.asarray(r['specularity']), 0.0).max(axis=0)
        cand = np.intersect1d(np.nonzero(sp >= 0.9 * sp.max())[0], active_modes(ct))
        act = cand[np.linspace(0, cand.shape[0] - 1, p['active']).astype(int)]
        m = np.arange(v.shape[0])
        out['degen_j2'] = np.where(m % 2 == 0, (m % J + 1) % J, -1).astype(np.int32)
    idle = np.nonzero(~((np.abs(v).max(axis=1) > 0) & (tau > 0)))[0]
    modes = np.concatenate([act[:2], idle[:1], act[2:], act[:1]]).astype(np.int32)
    lo, h, n = FD.grid_from_bounds(b, GOLDEN_GRID)
    lo = np.asarray(lo, dtype=np.float64) + 0.3 * np.asarray(h, dtype=np.float64)
    out.update(tau=tau, modes=modes, weight=case_weights(ct, modes)[1], lo=lo, h=np.asarray(h, dtype=np.float64), n_cells=np.asarray(n, dtype=np.int32))
    return out


def golden_case(name, inp):
    """The case's tables as the recorded calls use them (inp: golden_inputs, or the same read from the fixture)."""
    ct = case(GOLDEN[name]['case'])
    if 'degen_j2' in inp:
        ct = dict(ct, rough=dict(ct['rough'], degen_j2=np.asarray(inp['degen_j2'], dtype=np.int32)))
    return ct


MODE_KEYS = ('D', 'D2', 'T', 'hits', 'p_res', 'p_wall', 'w_left', 'p_int')
RAY_KEYS = ('ray_D', 'ray_T', 'ray_segments', 'ray_end', 'ray_x0')


def golden_calls(eng, name, inp):
    """The recorded calls on an engine with the case's tables, with n rays per mode and with one.  Returns (out, same): out, a flat
    dict of the arrays that are recorded -- <n>_x0 (drawn by the seed), <n>_paths_*, <n>_map_*, <n>_cols_* with <n> = 'n' or 'one'
    --, and same, {name: (array, key of out)}: the outputs that repeat a recorded array and are held against that one instead."""
    p = GOLDEN[name]
    tau, modes, kw = inp['tau'], inp['modes'], dict(max_segments=p['max_segments'], seed=p['seed'])
    out, same = {}, {}
    for tag, n in (('n', p['n']), ('one', 1)):
        x0 = eng.free_paths(tau, n=n, modes=modes, rays=True, **kw)['ray_x0']
        out[tag + '_x0'] = x0
        r = eng.free_paths(tau, n=n, modes=modes, x0=x0, rays=True, **kw)
        for k in MODE_KEYS + RAY_KEYS[:-1]:
            out['%s_paths_%s' % (tag, k)] = r[k]
        same[tag + '_paths_ray_x0'] = (r['ray_x0'], tag + '_x0')
        out[tag + '_paths_counts'] = np.array([r['report'][k] for k in ('rays', 'casts', 'missed', 'capped')], dtype=np.int64)
        r = eng.free_path_map(tau, inp['weight'], inp['lo'], inp['h'], inp['n_cells'], n=n, modes=modes, x0=x0, rays=True, **kw)
        for k in ('cells', 'ray_cell', 'ray_w'):
            out['%s_map_%s' % (tag, k)] = r[k]
        for k in MODE_KEYS + RAY_KEYS[:-1]:
            same['%s_map_%s' % (tag, k)] = (r[k], '%s_paths_%s' % (tag, k))
        same[tag + '_map_ray_x0'] = (r['ray_x0'], tag + '_x0')
        rep = r['report']
        out[tag + '_map_counts'] = np.array([rep[k] for k in ('rays', 'casts', 'missed', 'capped', 'clamped', 'overflow', 'k_K', 'k_P', 'k_T')], dtype=np.int64)
        out[tag + '_map_bounds'] = np.array([rep['B_K'], rep['B_T']])
        r = eng.free_path_columns(tau[None, :] * GOLDEN_COLUMNS[:, None], n=n, modes=modes, x0=x0, rays=True, **kw)
        for k in MODE_KEYS + ('casts', 'missed', 'capped'):
            out['%s_cols_%s' % (tag, k)] = r[k]
        out[tag + '_cols_shared'] = np.array([r['report']['casts_shared']], dtype=np.int64)
        for k in RAY_KEYS[:-1]:                             # column 4 has the factor 1: the plain call's rays
            same['%s_cols_%s_4' % (tag, k)] = (r[k][4], '%s_paths_%s' % (tag, k))
        same[tag + '_cols_ray_x0'] = (r['ray_x0'], tag + '_x0')
        out[tag + '_cols_ends'] = np.stack([np.bincount(e.ravel(), minlength=5) for e in r['ray_end']]).astype(np.int64)
    return out, same
