"""Free-path maps: the host side of Engine.free_path_map (nk_free_paths_map, k_free_map) -- NumPy only, usable without a GPU.

The engine flies the rays of free-path sampling (free_path.py) and bins every finished ray by the cell of its START point on
the field's grid (field.py): per cell the count N, the nine sums of w_a D_b (w = C_m v_m / (Q V) of the ray's list entry, D its
displacement), the final weights by the way the ray ended, and the flight time -- 64-bit integers that are the same bits in any
order of the rays.  From those this module forms the local conductivity

    kappa_ab(c) = sum over the rays that started in c of w_a D_b / (rays per mode in c)

for a mode set with inversion symmetry the backward flight of mode m from x is the forward flight of mode -m from x, so
sum_m C_m v_a E[D_b | x0 = x] is the local conductivity tensor at x in the relaxation-time picture (Fuchs-Sondheimer).  It is
exact on the terms that make the global estimate exact, and an approximation otherwise; in particular it carries the caveat
about reservoirs that end flights along the transport direction.  An ESTIMATE, not a replacement for the run's field.

Here: the option parser, the weights, the scales of the integers (the engine's report must agree), the integer tally restated
in NumPy (what the tests hold the GPU against, as field.quantised is for the field), the two normalisations, the closed form
averaged over a slab cell, and the writers / readers of free_path_map.npz and free_path_map.vtk.

Units are the package's: angstrom, ps, K, eV; conductivities in W/m K."""
import math
import os

import numpy as np

from . import field as FD
from . import free_path as FP

LINE = 16                      # NK_FREE_MAP_LINE: words of a cell's line
W_N, W_K, W_PRES, W_PWALL, W_WLEFT, W_T = 0, 1, 10, 11, 12, 13
KINDS = ('count', 'solid')


def free_path_map_option(value, free_path_n=None):
    """--free_path_map nx ny nz [count|solid] -> ((nx, ny, nz), kind), or (None, 'count') when off (the option is absent, or
    0 0 0).  free_path_n: the N of --free_path where the caller knows it; the map needs it (> 0)."""
    v = list(value) if isinstance(value, (list, tuple)) else ([] if value is None else [value])
    usage = '--free_path_map: expected nx ny nz [count|solid] (positive cell counts, at most 2^24 cells), got %r' % ' '.join(str(x) for x in v)
    if not v:
        return None, 'count'
    if len(v) not in (3, 4):
        raise ValueError(usage)
    try:
        n = tuple(int(x) for x in v[:3])
    except ValueError:
        raise ValueError(usage)
    kind = str(v[3]) if len(v) == 4 else 'count'
    if kind not in KINDS:
        raise ValueError(usage)
    if n == (0, 0, 0):
        return None, kind
    if min(n) <= 0 or n[0] * n[1] * n[2] > FD.MAX_CELLS:
        raise ValueError(usage)
    if free_path_n is not None and int(free_path_n) <= 0:
        raise ValueError('--free_path_map requires --free_path N [T] [max_segments]: the map bins the rays of that estimate')
    return n, kind


def weights(C, group_vel, qv):
    """w [L, 3] = C_m v_m / (Q V): the weight vectors of the modes of a list (C [L] from free_path.mode_heat_capacity, group_vel
    [L, 3]); kappa_ab = unit x sum over the modes of w_a mean(D_b)."""
    return np.asarray(C, dtype=np.float64).ravel()[:, None] * np.asarray(group_vel, dtype=np.float64).reshape(-1, 3) / float(qv)


def field_k(B, capacity):
    """nk_field_k (shared with the field and the mode tally): k = 62 - the binary exponent of capacity B, so that 2^61 <= capacity
    B 2^k < 2^62; within +-1000."""
    m = float(B) * float(max(int(capacity), 1))
    ex = math.frexp(m)[1]                   # m = f 2^ex, 0.5 <= f < 1
    return max(-1000, min(1000, 62 - ex))


def scales(weight, group_vel, tau, rays, capacity=0, weight_bound=0.0):
    """The scales of a call, the engine's rule: weight [L, 3] of the list, group_vel [M, 3] and tau [M] of ALL modes (reflections
    can change the mode), rays = L x n.  Over a ray sum W g <= 1, so with Lambda_max = the largest |v_m|_inf tau_m over the modes
    with tau > 0 and W_max = max(the largest |w|_inf, weight_bound): |w_a D_b| <= B_K = W_max Lambda_max, a final weight <= B_P = 1,
    a flight time <= B_T = the largest positive tau.  k = field_k(B, max(rays, capacity)).  dict k_K, k_P, k_T, B_K, B_T, cap."""
    w = np.asarray(weight, dtype=np.float64).reshape(-1, 3)
    v = np.asarray(group_vel, dtype=np.float64).reshape(-1, 3)
    t = np.asarray(tau, dtype=np.float64).ravel()
    live = t > 0
    lam = float(np.max(np.abs(v[live]).max(axis=1) * t[live])) if live.any() else 0.0
    tmax = float(t[live].max()) if live.any() else 0.0
    wmax = max(float(np.abs(w).max()) if w.size else 0.0, float(weight_bound))
    cap = max(int(rays), int(capacity))
    BK = wmax * lam
    return dict(k_K=field_k(BK, cap), k_P=field_k(1.0, cap), k_T=field_k(tmax, cap), B_K=BK, B_T=tmax, cap=cap)


def _q(term, k):
    """rint(term 2^k) as int64: round to nearest, ties to even."""
    return np.rint(np.ldexp(np.asarray(term, dtype=np.float64), int(k))).astype(np.int64)


def tally(x0, D, T, ray_w, end, weight_per_ray, lo, h, n, k_K, k_P, k_T):
    """The integer tally of the engine in NumPy -- the statement of the rule the GPU is held to.  Per ray: x0 [R, 3] its start
    point, D [R, 3], T [R], ray_w [R] the final weight that is routed (0 where none is), end [R] its end code, weight_per_ray
    [R, 3] the weight vector of its list entry.  Cell = field.cell_index (clamped into the grid).  -> cells [nx, ny, nz, 16]
    int64: word 0 the rays, 1 + 3a + b rint(w_a D_b 2^k_K), 10 / 11 / 12 rint(ray_w 2^k_P) by the end (1 reservoir -> 10, 2
    diffuse wall -> 11, 0 with weight left and 4 cap -> 12; a miss adds nothing), 13 rint(T 2^k_T), 14 and 15 zero.  Integer
    adds commute: any order of the rays gives the same bytes.  A term of exactly zero leaves no trace."""
    n = tuple(int(k) for k in n)
    x0 = np.asarray(x0, dtype=np.float64).reshape(-1, 3)
    D = np.asarray(D, dtype=np.float64).reshape(-1, 3)
    T = np.asarray(T, dtype=np.float64).ravel()
    rw = np.asarray(ray_w, dtype=np.float64).ravel()
    end = np.asarray(end, dtype=np.int64).ravel()
    w = np.asarray(weight_per_ray, dtype=np.float64).reshape(-1, 3)
    c, _ = FD.cell_index(x0, lo, h, n)
    q = (c[:, 0] * n[1] + c[:, 1]) * n[2] + c[:, 2]
    nc = n[0] * n[1] * n[2]
    cells = np.zeros((nc, LINE), dtype=np.int64)
    np.add.at(cells[:, W_N], q, 1)
    for a in range(3):
        for b in range(3):
            np.add.at(cells[:, W_K + 3 * a + b], q, _q(w[:, a] * D[:, b], k_K))
    qw = _q(rw, k_P)
    for word, sel in ((W_PRES, end == 1), (W_PWALL, end == 2), (W_WLEFT, (end == 0) | (end == 4))):
        np.add.at(cells[:, word], q[sel], qw[sel])
    np.add.at(cells[:, W_T], q, _q(T, k_T))
    return cells.reshape(n + (LINE,))


def sums(cells, report):
    """The reals the integers stand for: dict N [nx, ny, nz], S [.., 3, 3] (sum of w_a D_b), p_res, p_wall, w_left, T [..]."""
    c = np.asarray(cells)
    f = c.astype(np.float64)
    kK, kP, kT = int(report['k_K']), int(report['k_P']), int(report['k_T'])
    return dict(N=f[..., W_N], S=np.ldexp(f[..., W_K:W_K + 9], -kK).reshape(c.shape[:3] + (3, 3)), p_res=np.ldexp(f[..., W_PRES], -kP),
                p_wall=np.ldexp(f[..., W_PWALL], -kP), w_left=np.ldexp(f[..., W_WLEFT], -kP), T=np.ldexp(f[..., W_T], -kT))


def normalise(cells, report, n_samples, n_list, kind='count', solid_fraction=None, cell_volume=None, solid_volume=None, unit=None,
              kappa_bulk=None, axis=0):
    """The map per cell from the integers: dict
      kappa [nx, ny, nz, 3, 3] (W/m K; unit: free_path's factor eV / (ps angstrom K) -> W / (m K), the default),
      suppression [nx, ny, nz] = kappa_aa(cell) / kappa_bulk[a, a] along `axis` (NaN without kappa_bulk),
      N, and the shares p_res, p_wall, p_int, w_left of N (p_int = 1 - the others, the row invariant), T_mean the mean flight time.
    kind 'count': a cell's sums are divided by N_c / n_list, the observed rays per mode; NaN where N = 0.
    kind 'solid': by n_samples V_c,solid / V_solid, the expected rays per mode, with V_c,solid = solid_fraction x cell_volume
    (Engine.cell_solid_volume's exact volumes) and V_solid = solid_volume (default: their sum).  Unbiased: sum_c kappa(c)
    V_c,solid / V_solid is the global kappa of the same rays.  Cells with a fraction <= field.SOLID_EMPTY are NaN."""
    if kind not in KINDS:
        raise ValueError('normalise: kind must be count or solid')
    s = sums(cells, report)
    N = s['N']
    unit = FP._unit() if unit is None else float(unit)
    with np.errstate(divide='ignore', invalid='ignore'):
        if kind == 'count':
            per_mode = np.where(N > 0, N / float(n_list), np.nan)
        else:
            if solid_fraction is None or cell_volume is None:
                raise ValueError("normalise: 'solid' needs solid_fraction and cell_volume")
            fr = np.asarray(solid_fraction, dtype=np.float64)
            if fr.shape != N.shape:
                raise ValueError('normalise: solid_fraction must be shaped like the cells, %r, not %r' % (N.shape, fr.shape))
            Vc = np.where(fr > FD.SOLID_EMPTY, fr, 0.0) * float(cell_volume)
            Vs = float(Vc.sum()) if solid_volume is None else float(solid_volume)
            per_mode = np.where(Vc > 0, float(n_samples) * Vc / Vs, np.nan)
        kappa = unit * s['S'] / per_mode[..., None, None]
        Nn = np.where(N > 0, N, np.nan)
        shares = {k: s[k] / Nn for k in ('p_res', 'p_wall', 'w_left')}
        p_int = 1.0 - shares['p_res'] - shares['p_wall'] - shares['w_left']
        T_mean = s['T'] / Nn
        a = int(axis)
        if kappa_bulk is None:
            sup = np.full(N.shape, np.nan)
        else:
            sup = kappa[..., a, a] / float(np.asarray(kappa_bulk, dtype=np.float64)[a, a])
    return dict(kind=kind, axis=a, kappa=kappa, suppression=sup, N=N, p_res=shares['p_res'], p_wall=shares['p_wall'], p_int=p_int,
                w_left=shares['w_left'], T_mean=T_mean, rays_per_mode=per_mode)


def solid_mean(kappa, solid_fraction):
    """sum_c kappa(c) V_c,solid / V_solid over the cells with solid in them: with 'solid' the global tensor of the same rays."""
    fr = np.asarray(solid_fraction, dtype=np.float64)
    fr = np.where(fr > FD.SOLID_EMPTY, fr, 0.0)
    k = np.where(fr[..., None, None] > 0, np.asarray(kappa, dtype=np.float64), 0.0)
    return (k * fr[..., None, None]).sum(axis=(0, 1, 2)) / fr.sum()


def film_cell_suppression(mfp_x, L, x_lo, x_hi):
    """The closed form of free_path.film_suppression averaged over a slab cell.  Where only walls normal to x at x = 0 and
    x = L end the flights (box T T P), a ray of a mode with Lambda_x = v_x tau that starts at x0 has D_x = Lambda_x (1 -
    exp(-d / |Lambda_x|)), d the distance to the wall ahead (L - x0 for Lambda_x > 0, x0 for Lambda_x < 0).  Returns the mean of
    D_x / Lambda_x over x0 uniform in [x_lo, x_hi] (measured from the wall at 0), broadcast over the arguments: with d1 < d2 the
    distances of the cell's two faces and w = d2 - d1,
        1 - exp(-d1 / l) (1 - exp(-w / l)) / (w / l) = -expm1(-d1 / l) + exp(-d1 / l) [1 - (1 - exp(-w / l)) / (w / l)],
    both terms positive.  1 for Lambda_x = 0.  Its mean over cells that tile [0, L] is film_suppression(Lambda_x, L)."""
    lam = np.asarray(mfp_x, dtype=np.float64)
    a, b = np.asarray(x_lo, dtype=np.float64), np.asarray(x_hi, dtype=np.float64)
    lam, a, b = np.broadcast_arrays(lam, a, b)
    l = np.abs(lam)
    d1 = np.where(lam > 0, float(L) - b, a)
    w = b - a
    ok = l > 0
    ls = np.where(ok, l, 1.0)
    e1 = np.exp(-d1 / ls)
    out = -np.expm1(-d1 / ls) + e1 * one_minus_phi(w / ls)
    return np.where(ok, out, 1.0)


def one_minus_phi(u):
    """1 - (1 - exp(-u)) / u, u >= 0, without cancellation: below 1/2 the series u/2 - u^2/6 + u^3/24 - ... (22 terms: the
    next is below 1e-28 of the first), above the expression itself."""
    u = np.asarray(u, dtype=np.float64)
    small = u < 0.5
    us = np.where(small, u, 0.0)
    ser = np.zeros_like(us)
    for k in range(22, 0, -1):                       # Horner: sum_{k >= 1} (-1)^(k+1) u^k / (k + 1)!
        ser = us * ((1.0 if k % 2 else -1.0) / math.factorial(k + 1) + ser)
    ub = np.where(small, 1.0, u)
    return np.where(small, ser, 1.0 + np.expm1(-ub) / ub)


def film_profile(weight_x, mfp_x, L, x_lo, x_hi):
    """The closed form's suppression kappa_xx(cell) / kappa_bulk,xx of slab cells [x_lo, x_hi] (arrays [cells]) for modes with
    weights w_x [L] and Lambda_x [L]: sum_m w_x Lambda_x s_m(cell) / sum_m w_x Lambda_x."""
    wx = np.asarray(weight_x, dtype=np.float64).ravel()
    lam = np.asarray(mfp_x, dtype=np.float64).ravel()
    s = film_cell_suppression(lam[:, None], L, np.asarray(x_lo, dtype=np.float64)[None, :], np.asarray(x_hi, dtype=np.float64)[None, :])
    return ((wx * lam)[:, None] * s).sum(axis=0) / (wx * lam).sum()


# ------------------------------------------------------------------------------------------- files
def free_path_map_npz_path(folder):
    return os.path.join(folder, 'free_path_map.npz')


def free_path_map_vtk_path(folder):
    return os.path.join(folder, 'free_path_map.vtk')


_ARRAYS = ('kappa', 'suppression', 'N', 'p_res', 'p_wall', 'p_int', 'w_left', 'T_mean', 'rays_per_mode', 'cells')
_REPORT_INT = ('rays', 'casts', 'missed', 'capped', 'clamped', 'overflow', 'k_K', 'k_P', 'k_T', 'geometry_mode', 'calls', 'bytes')
_REPORT_REAL = ('B_K', 'B_T', 'seconds')


def write_free_path_map_npz(path, m):
    """free_path_map.npz from a map dict (normalise()'s plus lo, h, n, cells, report and, where known, solid_fraction,
    kappa_global, kappa_bulk, T, n_samples, n_list): every array, the grid, the scales and the report."""
    out = {k: np.asarray(m[k]) for k in _ARRAYS if k in m}
    out.update(lo=np.asarray(m['lo'], dtype=np.float64), h=np.asarray(m['h'], dtype=np.float64), n=np.asarray(m['n'], dtype=np.int64),
               kind=np.array(m['kind']), axis=np.int64(m['axis']))
    for k in ('solid_fraction', 'kappa_global', 'kappa_bulk'):
        if m.get(k) is not None:
            out[k] = np.asarray(m[k], dtype=np.float64)
    for k in ('T', 'n_samples', 'n_list'):
        if m.get(k) is not None:
            out[k] = np.float64(m[k]) if k == 'T' else np.int64(m[k])
    rep = m.get('report', {})
    for k in _REPORT_INT:
        if k in rep:
            out['report_' + k] = np.int64(rep[k])
    for k in _REPORT_REAL:
        if k in rep:
            out['report_' + k] = np.float64(rep[k])
    np.savez_compressed(path, **out)
    return path


def read_free_path_map_npz(path):
    """What write_free_path_map_npz wrote, with the report as a dict again."""
    with np.load(path) as z:
        raw = {k: z[k] for k in z.files}
    out, rep = {}, {}
    for k, v in raw.items():
        if k.startswith('report_'):
            rep[k[7:]] = int(v) if k[7:] in _REPORT_INT else float(v)
        elif k == 'kind':
            out[k] = str(v)
        elif k in ('axis', 'n_samples', 'n_list'):
            out[k] = int(v)
        elif k == 'T':
            out[k] = float(v)
        elif k == 'n':
            out[k] = tuple(int(x) for x in v)
        else:
            out[k] = v
    out['report'] = rep
    return out


def write_free_path_map_vtk(path, m, title='nanokappa free-path map'):
    """Legacy ASCII VTK in field.write_vtk's layout and cell order (it can be laid beside field.vtk): scalars N, kappa (along
    the axis), suppression and, where known, solid_fraction."""
    n = tuple(int(k) for k in m['n'])
    a = int(m['axis'])
    scalars = [('N', m['N']), ('kappa', np.asarray(m['kappa'])[..., a, a]), ('suppression', m['suppression'])]
    if m.get('solid_fraction') is not None:
        scalars.append(('solid_fraction', np.asarray(m['solid_fraction'], dtype=np.float64).reshape(n)))
    with open(path, 'w') as f:
        f.write('# vtk DataFile Version 3.0\n%s\nASCII\nDATASET STRUCTURED_POINTS\n' % title.replace('\n', ' ')[:255])
        f.write('DIMENSIONS %d %d %d\n' % (n[0] + 1, n[1] + 1, n[2] + 1))
        f.write('ORIGIN %.17g %.17g %.17g\n' % tuple(np.asarray(m['lo'], dtype=float)))
        f.write('SPACING %.17g %.17g %.17g\n' % tuple(np.asarray(m['h'], dtype=float)))
        f.write('CELL_DATA %d\n' % (n[0] * n[1] * n[2]))
        for name, arr in scalars:
            f.write('SCALARS %s double 1\nLOOKUP_TABLE default\n' % name)
            f.write('\n'.join('%.17g' % x for x in FD._vtk_order(np.asarray(arr, dtype=np.float64).reshape(n))) + '\n')
    return path


def read_free_path_map_vtk(path):
    """What write_free_path_map_vtk wrote (field.read_vtk reads the layout): dict lo, h, n, title, N, kappa, suppression
    (nx, ny, nz) and solid_fraction where the file holds it."""
    return FD.read_vtk(path)
