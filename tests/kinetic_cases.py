"""Kinetic flights on the CPU: the rule of nk_kinetic_flights (DESIGN.md "Kinetic flights") restated in NumPy, vectorised over the
rays, with the oracle's ray cast (nko_find_boundary), its classifier (nko_classify) and its random numbers (Philox4x32-10 restated
here over arrays; test_kinetic_host.py holds it against nko_uniform2).  The rule stands here once, for all three entries: restate()
is the plain call, restate(groups=...) adds the group tally of nk_kinetic_flights_groups and restate(grids=...) the map tally of
nk_kinetic_flights_map to the same loop (kinetic_group_cases.py and kinetic_map_cases.py name their results).  What the GPU tests
hold the kernel against, and the cases they share.  Test infrastructure: nothing under nanokappa_amd/ knows of it.

The draws (nanokappa_amd/csrc/nk_kinetic.h), all uniform2(seed, ray id, k, tag) -> (a, b), ray id = (source << 32) | sample, k = the
ray's event count when the draw is made:
    TAG_KIN + 0       k = 0: a the triangle of the source facet (searchsorted right on its cumulative areas), sqrt(b) the first weight
    TAG_KIN + 1       k = 0: a the second barycentric draw
    TAG_KIN + 2       a segment: a the free time t_s = -tau ln(a) (a = 0 -> 2^-54), b the point on the segment
    TAG_KIN + 3       a scattering (k = the event's number, from 1): a draws the mode from cdf_scatter
    TAG_KIN + 64 + j  trial j < 64 of an emission (k = 0) or re-emission (k = the event's number): a draws the mode from cdf_flux,
                      accepted iff b |v| < (v . n_in)+
    TAG_FREE + 3      a rough facet's specular test, the free-path flight's own (k = the event's number)."""
import ctypes as C

import numpy as np

import free_path_cases as FC
from free_path_cases import O, cached, fma

TAG_KIN = 0x60000
TAG_FREE = FC.TAG_FREE
TRIALS = 64
MAX_EVENTS = 2 ** 20
END_LOST, END_MISSED, END_CAPPED = -1, -2, -3
ROW_WORDS = 32
_M32 = np.uint64(0xFFFFFFFF)


def uniform2(seed, pid, step, tag):
    """nk_uniform2_dev / nko_uniform2 over arrays: Philox4x32-10, counter {pid lo, pid hi, step, tag}, key = seed."""
    pid = np.asarray(pid, dtype=np.uint64)
    c0, c1 = pid & _M32, pid >> np.uint64(32)
    c2 = np.broadcast_to(np.asarray(step, dtype=np.uint64), pid.shape).copy()
    c3 = np.broadcast_to(np.asarray(tag, dtype=np.uint64), pid.shape).copy()
    k0, k1 = np.uint64(int(seed) & 0xFFFFFFFF), np.uint64((int(seed) >> 32) & 0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        n0, n2 = (p1 >> np.uint64(32)) ^ c1 ^ k0, (p0 >> np.uint64(32)) ^ c3 ^ k1
        c0, c1, c2, c3 = n0, p1 & _M32, n2, p0 & _M32
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & _M32, (k1 + np.uint64(0xBB67AE85)) & _M32
    u = lambda hi, lo: (((hi << np.uint64(32)) | lo) >> np.uint64(11)).astype(np.float64) * (1.0 / 9007199254740992.0)
    return u(c0, c1), u(c2, c3)


def classify(sv, x):
    x = np.ascontiguousarray(x, dtype=np.float64)
    out = np.zeros(x.shape[0], dtype=np.int32)
    O.lib().nko_classify(C.byref(sv), C.c_int64(x.shape[0]), x.ctypes.data_as(O.c_dp), out.ctypes.data_as(O.c_ip))
    return out.astype(np.int64)


def facet_faces(g):
    """(offsets [Fc + 1], face indices, cumulative area fractions): nk_set_mesh's tables of a facet's faces."""
    if 'facets_flat' in g:
        flat, ln = np.asarray(g['facets_flat'], dtype=int), np.asarray(g['facets_len'], dtype=int)
    else:
        flat, ln = np.concatenate(g['facets']).astype(int), np.array([len(f) for f in g['facets']])
    off = np.concatenate(([0], np.cumsum(ln)))
    area = np.asarray(g['face_areas'], dtype=np.float64)
    cdf = np.zeros(flat.shape[0])
    for fc in range(ln.shape[0]):
        tot = 0.0
        for a in range(off[fc], off[fc + 1]):
            tot += area[flat[a]]
        acc = 0.0
        for a in range(off[fc], off[fc + 1]):
            acc += area[flat[a]] / tot
            cdf[a] = acc
        cdf[off[fc]:off[fc + 1]] /= cdf[off[fc + 1] - 1]
    return off, flat, cdf


def _pos(t, v, x, fused):
    return fma(t[:, None], v, x) if fused else x + t[:, None] * v


def _emit(seed, rid, k, n_in, vg, cdf_flux, cosine=True):
    """The rejection rule for the rays (rid, k) with inward normals n_in [R, 3]: (mode [R], -1 where lost)."""
    R = rid.shape[0]
    mode = -np.ones(R, dtype=np.int64)
    todo = np.arange(R)
    M = vg.shape[0]
    for j in range(TRIALS):
        if not todo.size:
            break
        u0, u1 = uniform2(seed, rid[todo], k[todo], TAG_KIN + 64 + j)
        m = np.minimum(np.searchsorted(cdf_flux, u0, side='right'), M - 1)
        v, n = vg[m], n_in[todo]
        vn = (v[:, 0] * n[:, 0] + v[:, 1] * n[:, 1]) + v[:, 2] * n[:, 2]
        sp = np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])
        ok = (u1 * sp < vn) if cosine else (vn > 0)
        mode[todo[ok]] = m[ok]
        todo = todo[~ok]
    return mode


def _q(term, s, B):
    """rint(term s) as int64 where |term| <= B, else 0; and the count of the terms left out."""
    term = np.asarray(term, dtype=np.float64)
    ok = np.abs(term) <= B
    return np.where(ok, np.rint(np.where(ok, term, 0.0) * s), 0.0).astype(np.int64), int((~ok).sum())


def _over(term, B, src, F):
    """The count of the terms _q leaves out, by source [F]: src holds the source of every term."""
    return np.bincount(np.asarray(src)[~(np.abs(np.asarray(term, dtype=np.float64)) <= B)], minlength=F).astype(np.int64)


def columns(table, G):
    """The column of every mode in a group tally: its group, or G (the rest column) where the table holds -1."""
    t = np.asarray(table, dtype=np.int64).ravel()
    assert t.min() >= -1 and t.max() < G
    return np.where(t < 0, int(G), t)


def bounds(g, tau, vg, cdf_scatter, n, max_events):
    """nk_kinetic_flights' bounds and scales: dict B_t, B_x, k_t, k_x, k_T, k_D, k_D2 (and the per-ray bounds BT, BD, BD2)."""
    b = np.asarray(g['bounds'], dtype=np.float64).reshape(2, 3)
    e = b[1] - b[0]
    diag = np.sqrt(e[0] * e[0] + e[1] * e[1] + e[2] * e[2])
    live = np.diff(np.concatenate(([0.0], cdf_scatter))) > 0
    sp = np.sqrt(vg[:, 0] * vg[:, 0] + vg[:, 1] * vg[:, 1] + vg[:, 2] * vg[:, 2])
    with np.errstate(divide='ignore', over='ignore'):
        tb = np.where(sp > 0, np.minimum(38.0 * tau, 2.0 * diag / np.where(sp > 0, sp, 1.0)), 38.0 * tau)
    Bt = float(tb[live].max())
    Bx = max(float((tb * np.abs(vg).max(axis=1))[live].max()), 1e-300)
    k = lambda B, cap: 62 - int(np.frexp(B * float(max(cap, 1)))[1])
    out = dict(B_t=Bt, B_x=Bx, BT=1024.0 * Bt, BD=1024.0 * Bx, BD2=(32.0 * Bx) * (32.0 * Bx))
    cap = n * max_events
    out.update(k_t=k(Bt, cap), k_x=k(Bx, cap), k_T=k(out['BT'], n), k_D=k(out['BD'], n), k_D2=k(out['BD2'], n))
    return out


def restate(g, sv, group_vel, tau, c, n, seed=0, max_events=MAX_EVENTS, rough=None, J=None, fused=True, cosine=True, tallies=True, trace=None,
            groups=(), grids=()):
    """The rule for n rays from every 'T' facet of the mesh tables g.  sv: the oracle's subvolume struct; c [M] the volumetric heat
    capacities; rough as free_path_cases.restate.  fused: positions by one fused multiply-add (the kernel's) or by a product and a
    sum.  cosine=False switches the cosine rejection off (any mode that flies inwards is accepted): the power check of the
    isothermal test.  trace: a dict that receives the counts of the segments sat out in a mode with v = 0 ('sitting'), of the specular
    turns ('turns'), of those into a mode with tau <= 0 ('dead_turns') and of the segments' terms left out, over all sources ('left_out_t',
    'left_out_x').  Returns the dict of Engine.kinetic_flights with rays=True
    (without `report`'s device figures).
    groups: a sequence of (table, G) -- a segment's four integers also go to (source, subvolume, column of the mode the segment was
    flown in) of every table (DESIGN.md "Kinetic groups"); the dict then holds `groups`, the list of their [F, S, G + 1, 4] int64.
    grids: a sequence of ((lo, h, n_cells), start_point) -- the four integers also go to (source, cell of the segment's point x_p) on
    every grid, the cell by nanokappa_amd.field.cell_index (DESIGN.md "Kinetic maps"); start_point=True bins the segment's START
    point x instead: the WRONG rule, for the sensitivity check of the isothermal test.  The dict then holds `grids`, the list of
    (map [F, nx, ny, nz, 4] int64, clamped [F]).  kinetic_group_cases.restate_grouped and kinetic_map_cases.restate_map name them."""
    from nanokappa_amd import field as FD
    from nanokappa_amd import kinetic as KN
    mesh = O.make_mesh(g)
    vg = np.asarray(group_vel, dtype=np.float64).reshape(-1, 3)
    tau = np.asarray(tau, dtype=np.float64).ravel()
    M = vg.shape[0]
    cs, cf = KN.tables(c, tau, vg)
    bc, trans, ridx = FC.facet_tables(g, rough)
    src = KN.source_facets(g['bound_cond'])
    F = src.shape[0]
    S = int(sv.S)
    src_of = -np.ones(bc.shape[0], dtype=np.int64)
    src_of[src] = np.arange(F)
    off, flat, fcdf = facet_faces(g)
    verts = np.asarray(g['vertices'], dtype=np.float64)[np.asarray(g['faces'], dtype=int)]          # [F, 3, 3]
    n_in_facet = -np.asarray(g['facets_normal'], dtype=np.float64)
    bd = bounds(g, tau, vg, cs, n, max_events)
    st, sx = 2.0 ** bd['k_t'], 2.0 ** bd['k_x']
    R = F * n
    sidx = np.repeat(np.arange(F), n)
    rid = (sidx.astype(np.uint64) << np.uint64(32)) | np.tile(np.arange(n, dtype=np.uint64), F)
    zero = np.zeros(R, dtype=np.int64)
    assert tallies or not (groups or grids)
    gt = [(columns(t_, G_), np.zeros((F, S, int(G_) + 1, 4), dtype=np.int64)) for t_, G_ in groups]      # (column of every mode, grp)
    mt = []                                                 # (lo, h, n_cells, start_point, map [F, ncells, 4], clamped [F])
    for (lo_, h_, n_), sp_ in grids:
        n_ = tuple(int(k_) for k_ in n_)
        mt.append((np.asarray(lo_, dtype=np.float64), np.asarray(h_, dtype=np.float64), n_, bool(sp_),
                   np.zeros((F, n_[0] * n_[1] * n_[2], 4), dtype=np.int64), np.zeros(F, dtype=np.int64)))
    # emission
    uf, us = uniform2(seed, rid, zero, TAG_KIN + 0)
    ur, _ = uniform2(seed, rid, zero, TAG_KIN + 1)
    x = np.zeros((R, 3))
    for f in range(F):
        r = np.nonzero(sidx == f)[0]
        f0, nf = off[src[f]], off[src[f] + 1] - off[src[f]]
        a = np.minimum(np.searchsorted(fcdf[f0:f0 + nf], uf[r], side='right'), nf - 1)
        fv = verts[flat[f0 + a]]
        sq = np.sqrt(us[r])
        a0, a1, a2 = 1.0 - sq, (1.0 - ur[r]) * sq, ur[r] * sq
        x[r] = (a0[:, None] * fv[:, 0] + a1[:, None] * fv[:, 1]) + a2[:, None] * fv[:, 2]
    x0 = x.copy()
    mode = _emit(seed, rid, zero, n_in_facet[src[sidx]], vg, cf, cosine)
    mode0 = mode.copy()
    end = np.where(mode < 0, END_LOST, 0).astype(np.int64)
    k, ncast = np.zeros(R, dtype=np.int64), np.zeros(R, dtype=np.int64)
    D, T = np.zeros((R, 3)), np.zeros(R)
    hsh = np.zeros(R, dtype=np.uint64)
    sub = np.zeros((F, S, 4), dtype=np.int64)
    ovSt, ovSx = np.zeros(F, dtype=np.int64), np.zeros(F, dtype=np.int64)       # the segments' terms left out, by source
    act = np.nonzero(mode >= 0)[0]
    seen = dict(sitting=0, turns=0, dead_turns=0, left_out_t=0, left_out_x=0)
    while act.size:
        m = mode[act]
        v, t_m = vg[m], tau[m]
        u, up = uniform2(seed, rid[act], k[act], TAG_KIN + 2)
        u = np.where(u > 0.0, u, 2.0 ** -54)
        ts = -t_m * np.log(u)
        flies = (v != 0).any(axis=1)
        tc, fc = np.full(act.shape[0], np.inf), -np.ones(act.shape[0], dtype=np.int64)
        if flies.any():
            a, b = FC.find_boundary(mesh, x[act[flies]], v[flies])
            tc[flies], fc[flies] = a, b
            ncast[act[flies]] += 1
        miss = flies & (fc < 0)
        end[act[miss]] = END_MISSED
        go = ~miss
        i, v, ts, tc, fc, up, flies, m = act[go], v[go], ts[go], tc[go], fc[go], up[go], flies[go], m[go]
        scat = ~flies | (ts < tc)
        seen['sitting'] += int((~flies).sum())
        t = np.where(scat, ts, tc)
        D[i] = fma(t[:, None], v, D[i])
        T[i] = T[i] + t
        if tallies:
            xp = _pos(up * t, v, x[i], fused)               # the one uniform point of the segment: subvolume AND cell
            s = classify(sv, xp)
            qt, o = _q(t, st, bd['B_t'])
            seen['left_out_t'] += o
            ovSt += _over(t, bd['B_t'], sidx[i], F)
            q4 = [qt]
            for a in range(3):
                qa, o = _q(t * v[:, a], sx, bd['B_x'])
                seen['left_out_x'] += o
                ovSx += _over(t * v[:, a], bd['B_x'], sidx[i], F)
                q4.append(qa)
            for w in range(4):
                np.add.at(sub[:, :, w], (sidx[i], s), q4[w])
                for col, grp in gt:                         # m: the mode the segment was flown in (the event below may change it)
                    np.add.at(grp[:, :, :, w], (sidx[i], s, col[m]), q4[w])
            for lo_, h_, n_, sp_, mp, cl in mt:
                ci, out = FD.cell_index(x[i] if sp_ else xp, lo_, h_, n_)
                cell = (ci[:, 0] * n_[1] + ci[:, 1]) * n_[2] + ci[:, 2]
                for w in range(4):
                    np.add.at(mp[:, :, w], (sidx[i], cell), q4[w])
                cl += np.bincount(sidx[i][out], minlength=F)
        k[i] += 1
        hp = _pos(t, v, x[i], fused)
        hsh[i] = hsh[i] * np.uint64(1000003) + np.where(scat, 1, fc + 2).astype(np.uint64)
        now = scat.copy()                                   # rays that draw a new mode from cdf_scatter at this event
        x[i[scat]] = hp[scat]
        alive = np.ones(i.shape[0], dtype=bool)
        b = np.where(scat, 0, bc[np.maximum(fc, 0)])
        res = b == ord('T')
        end[i[res]] = src_of[fc[res]]
        alive[res] = False
        per = b == ord('P')
        x[i[per]] = hp[per] + trans[fc[per]]
        ro = np.nonzero(b == ord('R'))[0]
        if ro.size:
            r0, r1 = uniform2(seed, rid[i[ro]], k[i[ro]], TAG_FREE + 3)
            f = ridx[fc[ro]]
            mr = mode[i[ro]]
            out = np.where(f >= 0, np.asarray(rough['spec_map'])[np.maximum(f, 0), mr], -1).astype(np.int64)
            spec = (f >= 0) & np.asarray(rough['true_spec'])[np.maximum(f, 0), mr].astype(bool) & \
                (r0 <= np.asarray(rough['specularity'])[np.maximum(f, 0), mr]) & (out >= 0) & (out < M)
            x[i[ro]] = hp[ro]
            dj = rough.get('degen_j2')
            if dj is not None:
                j2 = np.asarray(dj, dtype=np.int64)[np.maximum(out, 0)]
                out = np.where(spec & (j2 > -1) & (j2 < J) & (r1 >= 0.5), (out // J) * J + j2, out)
            sp_i = ro[spec]
            mode[i[sp_i]] = out[spec]
            now[sp_i] = ~(tau[out[spec]] > 0.0)
            seen['turns'] += int(sp_i.size)
            seen['dead_turns'] += int(now[sp_i].sum())
            df = ro[~spec]
            if df.size:
                mnew = _emit(seed, rid[i[df]], k[i[df]], n_in_facet[fc[df]], vg, cf, cosine)
                mode[i[df]] = mnew
                lost = mnew < 0
                end[i[df[lost]]] = END_LOST
                alive[df[lost]] = False
        if now.any():
            us2, _ = uniform2(seed, rid[i[now]], k[i[now]], TAG_KIN + 3)
            mode[i[now]] = np.minimum(np.searchsorted(cs, us2, side='right'), M - 1)
        cap = alive & (k[i] >= max_events)
        end[i[cap]] = END_CAPPED
        alive[cap] = False
        act = i[alive]
    if trace is not None:
        trace.update(seen)
    # the sums of the finished rays
    rows = np.zeros((F, ROW_WORDS), dtype=np.int64)
    sD, sD2, sT = 2.0 ** bd['k_D'], 2.0 ** bd['k_D2'], 2.0 ** bd['k_T']
    for f in range(F):
        r = sidx == f
        for e in range(F):
            rows[f, e] = int((end[r] == e).sum())
        rows[f, 8], rows[f, 9], rows[f, 10] = (int((end[r] == c_).sum()) for c_ in (END_LOST, END_MISSED, END_CAPPED))
        rows[f, 11], rows[f, 12] = int(k[r].sum()), int(ncast[r].sum())
        for a in range(3):
            q, o = _q(D[r, a], sD, bd['BD'])
            rows[f, 13 + a], rows[f, 20] = q.sum(), rows[f, 20] + o
            q, o = _q(D[r, a] * D[r, a], sD2, bd['BD2'])
            rows[f, 16 + a], rows[f, 21] = q.sum(), rows[f, 21] + o
        q, o = _q(T[r], sT, bd['BT'])
        rows[f, 19], rows[f, 22] = q.sum(), o
    rows[:, 23], rows[:, 24] = ovSt, ovSx
    sh = (F, n)
    rep = dict(bd, rays=R, events=int(k.sum()), casts=int(ncast.sum()), lost=int((end == END_LOST).sum()), missed=int((end == END_MISSED).sum()),
               capped=int((end == END_CAPPED).sum()), overflow=int(rows[:, 20:25].sum()), n_sources=F, n_subvolumes=S, source_facet=list(src))
    res = dict(n=n, source_facet=src, ends=rows[:, :F].copy(), lost=rows[:, 8].copy(), missed=rows[:, 9].copy(), capped=rows[:, 10].copy(),
               events=rows[:, 11].copy(), casts=rows[:, 12].copy(), D=rows[:, 13:16] / sD, D2=rows[:, 16:19] / sD2, dwell_total=rows[:, 19] / sT,
               dwell=sub[:, :, 0] / st, flux=sub[:, :, 1:4] / sx, rows=rows, sub=sub, cdf_scatter=cs, cdf_flux=cf, report=rep,
               ray_x0=x0.reshape(sh + (3,)), ray_mode=mode0.reshape(sh).astype(np.int32), ray_end=end.reshape(sh).astype(np.int32),
               ray_events=k.reshape(sh).astype(np.int32), ray_casts=ncast.reshape(sh).astype(np.int32), ray_D=D.reshape(sh + (3,)),
               ray_dwell=T.reshape(sh), ray_hash=hsh.reshape(sh))
    if gt:
        res['groups'] = [t_[1] for t_ in gt]
    if mt:
        res['grids'] = [(t_[4].reshape((F,) + t_[2] + (4,)), t_[5]) for t_ in mt]
    return res


# ------------------------------------------------------------------------------------------- cases
T_CASE = FC.T_CASE
BOX3_ARGS = ['--geometry', 'box', '--dimensions', '300', '200', '100', '--subvolumes', 'slice', '6', '0',
             '--bound_pos', 'relative', '0', '.5', '.5', '1', '.5', '.5', '.5', '0', '.5',
             '--bound_cond', 'T', 'T', 'T', 'R', '--bound_values', '302', '298', '300', '5']


def case(name):
    """free_path_cases.case's cases plus 'box3': the three-terminal box 300 x 200 x 100 A, 'T' on x-, x+ and y-, 'R' elsewhere."""
    if name != 'box3':
        return FC.case(name)

    def make():
        from edge_cases import COMMON_ARGS
        from util import case_from_args
        return case_from_args(BOX3_ARGS + COMMON_ARGS)
    return cached(('kin_case', name), make)


def subvols(ct):
    from util import sv_interp_of
    kind = ct.get('kind', 0)
    itp, rbf = sv_interp_of(ct, kind, 1)
    return O.make_subvols(ct['centers'], ct['volumes'], kind, ct['axis'], itp, rbf=rbf)


def heat_capacity(ct, T=T_CASE):
    from nanokappa_amd import kinetic as KN
    ph = ct['ph']
    return KN.heat_capacity(ph.omega, T, ph.number_of_qpoints * ph.volume_unitcell)


def lifetimes(ct, scale=1.0, T=T_CASE):
    """tau [M] at T, times `scale` (a power of two) where positive; scale = inf: the ballistic limit, 1e30 where a mode lives."""
    tau = FC.lifetimes(ct, T)
    if np.isinf(scale):
        return np.where(tau > 0, 1e30, tau)
    return np.where(tau > 0, tau * scale, tau)


def run_case(name, n, seed, scale=1.0, max_events=MAX_EVENTS, fused=True, cosine=True, tallies=True):
    """The restatement on a named case (cached by all its arguments)."""
    def make():
        ct = case(name)
        return restate(ct['mesh'], subvols(ct), FC.group_vel(ct), lifetimes(ct, scale), heat_capacity(ct), n, seed=seed, max_events=max_events,
                       rough=ct['rough'], J=ct['J'], fused=fused, cosine=cosine, tallies=tallies)
    return cached(('kin_run', name, n, seed, scale, max_events, fused, cosine, tallies), make)


def engine_for(ct, seed=7):
    """An engine with the case's tables and a few particles (the calls do not touch them)."""
    from util import make_engine, random_population, population_in_mesh
    pos, mode, occ, counter = (population_in_mesh if 'geo' in ct else random_population)(ct, 2000, seed=3)
    return make_engine(ct, pos, mode, occ, counter, seed=seed)


def source_geometry(ct):
    """(source facets, areas [F], inward normals [F, 3], centroids) of a case's 'T' facets."""
    from nanokappa_amd import kinetic as KN
    g = ct['mesh']
    src = KN.source_facets(g['bound_cond'])
    off, flat, _ = facet_faces(g)
    area = np.array([np.asarray(g['face_areas'], dtype=float)[flat[off[f]:off[f + 1]]].sum() for f in src])
    return src, area, -np.asarray(g['facets_normal'], dtype=float)[src], np.asarray(g['facet_centroid'], dtype=float)[src]


# Ray by ray, kernel against restatement (tests/test_gpu_kinetic.py): name -> case, lifetime scale, seed; 2 sources x 256 rays each
PARITY = {
    'ttp': dict(case='ttp', scale=1.0, seed=41),
    'ttp_16': dict(case='ttp', scale=1.0 / 16.0, seed=42),               # tens of scatterings per ray
    'ttrrp_k': dict(case='ttrrp_k', scale=1.0, seed=43),                 # specular turns and diffuse re-emission
    'wire72': dict(case='wire72', scale=1.0, seed=44),                   # the tree cast, tilted normals
}
PARITY_N = 256
# The statistical tests: 8 seeds and N rays per source, chosen on the CPU so that the restatement passes them (the engine then flies
# the same rays).  A bound of 5 standard errors taken from 8 calls is a Student-t bound with 7 degrees of freedom, which one of the
# tens of subvolume means exceeds by chance in about one set of seeds out of ten; 32 seeds x 8192 rays show no bias (every mean
# within 2.5 standard errors of 0.6 %).
STAT = {
    'ttp_16': dict(case='ttp', scale=1.0 / 16.0, n=8192, seeds=tuple(range(200, 208))),
    'box3': dict(case='box3', scale=1.0, n=4096, seeds=tuple(range(101, 109))),
}


def stat_runs(name, cosine=True):
    """The restatement's 8 calls of a statistical case (cached; callers must not modify them)."""
    p = STAT[name]
    return [run_case(p['case'], p['n'], s, scale=p['scale'], cosine=cosine) for s in p['seeds']]


def stat_inputs(name):
    p = STAT[name]
    ct = case(p['case'])
    return ct, lifetimes(ct, p['scale'])


def parity_run(name, fused=True):
    p = PARITY[name]
    return run_case(p['case'], PARITY_N, p['seed'], scale=p['scale'], fused=fused)


def isothermal(res, ct, tau):
    """dT_s [S] (K) and q_s [S, 3] (W/m^2) of a result with every source 1 K above the reference: 1 and 0 in the exact solution."""
    from nanokappa_amd import kinetic as KN
    c = heat_capacity(ct)
    lv = KN.live_modes(c, tau)
    src, area, n_in, _ = source_geometry(ct)
    g = KN.source_strength(area, n_in, c, FC.group_vel(ct), lv)
    import math
    return KN.profile(res, g, np.ones(src.shape[0]), ct['volumes'], math.fsum(c[lv]))


# ------------------------------------------------------------------------------------------- the statistical checks
# Shared by test_kinetic_host.py (on the restatement) and test_gpu_kinetic.py (on the engine, which flies the same rays): each takes
# the results of the calls with STAT_SEEDS.  A mean over the seeds is held within 5 standard errors taken from the 8 calls.
def mean_se(a):
    a = np.asarray(a, dtype=np.float64)
    return a.mean(axis=0), a.std(axis=0, ddof=1) / np.sqrt(a.shape[0])


def isothermal_deviation(results, ct, tau):
    """(worst |mean dT - 1| / se, worst se of dT, worst |mean q| / se) over the subvolumes, every source 1 K above the reference."""
    dT, q = zip(*(isothermal(r, ct, tau) for r in results))
    m, se = mean_se(dT)
    mq, sq = mean_se(q)
    return float(np.max(np.abs(m - 1.0) / se)), float(se.max()), float(np.max(np.abs(mq) / sq))


def conductances(results, ct, tau):
    """(G [F, F], its binomial standard error) in W/K from the pooled counts of the calls."""
    from nanokappa_amd import kinetic as KN
    c = heat_capacity(ct)
    src, area, n_in, _ = source_geometry(ct)
    g = KN.source_strength(area, n_in, c, FC.group_vel(ct), KN.live_modes(c, tau))
    T, se = KN.transmission(sum(r['ends'] for r in results), sum(r['n'] for r in results))
    return g[:, None] * T, g[:, None] * se, g


def reciprocity_deviation(results, ct, tau):
    """worst |G_fg - G_gf| / its binomial standard error over the pairs f < g."""
    G, se, _ = conductances(results, ct, tau)
    F = G.shape[0]
    return max(abs(G[f, g] - G[g, f]) / np.hypot(se[f, g], se[g, f]) for f in range(F) for g in range(f + 1, F))


def flux_deviation(results, ct, tau, axis=0, dT=4.0):
    """On two facing reservoirs at T_ref +- dT / 2: (worst |mean(q_axis - G_01 dT / A)| / se over the slices, worst |mean q_other| / se)."""
    from nanokappa_amd import kinetic as KN
    from nanokappa_amd.constants import Constants
    c = heat_capacity(ct)
    lv = KN.live_modes(c, tau)
    src, area, n_in, _ = source_geometry(ct)
    g = KN.source_strength(area, n_in, c, FC.group_vel(ct), lv)
    a = Constants().a_in_m
    diff, other = [], []
    for r in results:
        _, q = KN.profile(r, g, np.array([0.5 * dT, -0.5 * dT]), ct['volumes'], 1.0)
        T, _ = KN.transmission(r['ends'], r['n'])
        G01 = 0.5 * (g[0] * T[0, 1] + g[1] * T[1, 0])
        sign = 1.0 if n_in[0][axis] > 0 else -1.0
        diff.append(q[:, axis] - sign * G01 * dT / (area[0] * a * a))
        other.append(np.delete(q, axis, axis=1))
    m, se = mean_se(diff)
    mo, so = mean_se(other)
    return float(np.max(np.abs(m) / se)), float(np.max(np.abs(mo) / so)), float(np.mean(se) / abs(G01 * dT / (area[0] * a * a)))
