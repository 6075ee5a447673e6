"""Free-path sweeps: the host side of Engine.free_path_columns (nk_free_paths_columns, k_free_columns) -- NumPy only, usable
without a GPU.

The path of a ray of the free-path rule (free_path.py) does not depend on the lifetimes, so the engine casts every ray once and
weighs it with K lifetime tables.  Two curves come out of one set of casts:

    scale s         the structure scaled by s with unchanged roughness is the same flight with hit times s tc, so a = tc / (tau / s):
                    with the lifetimes tau / s on the unscaled mesh the displacement of the scaled structure is D_s = s D' (its
                    squares s^2 D'^2, flight times and mean free paths s times those of the column).  columns_scale gives tau / s,
                    scaled_column multiplies back: column c IS the structure scaled by s_c at the lifetimes tau.
    temperature T   enters through tau(T) (columns_temperature) and, in the summary, through C_m(T).

An ESTIMATE in every column, as free_path.py says.  Units are the package's: angstrom, ps, K, eV; conductivities in W/m K."""
import os

import numpy as np

from . import free_path as FP
from . import modes as MD

MAX_COLUMNS = 32              # NK_FREE_PATH_MAX_COLUMNS (include/nanokappa_hip.h)
KINDS = ('scale', 'temperature')
SUM_KEYS = ('D', 'D2', 'T', 'hits', 'p_res', 'p_wall', 'w_left', 'p_int')


def sweep_option(value, free_path_n=0):
    """--free_path_sweep scale s1 s2 ... | temperature T1 T2 ... -> (kind, values [K]); (None, None) when the option is absent.
    The values must be finite and > 0, at most MAX_COLUMNS of them, and --free_path N must be on (free_path_n > 0)."""
    if value is None:
        return None, None
    v = list(value) if isinstance(value, (list, tuple)) else [value]
    if len(v) == 0:
        return None, None
    usage = ('--free_path_sweep: expected scale s1 s2 ... or temperature T1 T2 ... (1 to %d finite values > 0; needs --free_path N), got %r'
             % (MAX_COLUMNS, ' '.join(str(x) for x in v)))
    kind = str(v[0])
    if kind not in KINDS or len(v) < 2 or len(v) - 1 > MAX_COLUMNS:
        raise ValueError(usage)
    try:
        vals = np.array([float(x) for x in v[1:]], dtype=np.float64)
    except ValueError:
        raise ValueError(usage)
    if not np.all(np.isfinite(vals) & (vals > 0)) or not int(free_path_n) > 0:
        raise ValueError(usage)
    return kind, vals


def columns_scale(tau, scales):
    """taus [K, M] = tau / s_c: the lifetimes with which the unscaled mesh flies the structure scaled by s_c."""
    s = np.asarray(scales, dtype=np.float64).ravel()
    return np.asarray(tau, dtype=np.float64).ravel()[None, :] / s[:, None]


def columns_temperature(phonon, temperatures):
    """taus [K, M] = free_path.lifetimes(phonon, T_c)."""
    return np.stack([FP.lifetimes(phonon, float(T)) for T in np.asarray(temperatures, dtype=np.float64).ravel()])


def column(res, c):
    """Column c of an Engine.free_path_columns result (or of results stacked like it) in the shape of an Engine.free_paths result."""
    out = {k: np.asarray(res[k])[c] for k in SUM_KEYS}
    for k in ('ray_D', 'ray_T', 'ray_segments', 'ray_end'):
        if k in res:
            out[k] = np.asarray(res[k])[c]
    if 'ray_x0' in res:
        out['ray_x0'] = res['ray_x0']
    rep = dict(res.get('report', {}))
    rep.update(casts=int(res['casts'][c]), missed=int(res['missed'][c]), capped=int(res['capped'][c]))
    out.update(modes=res['modes'], n=res['n'], report=rep)
    return out


def stack(results):
    """K free_paths-shaped results on one list (Engine.free_paths, or the tests' restatement) as one free_path_columns-shaped result."""
    out = {k: np.stack([np.asarray(r[k]) for r in results]) for k in SUM_KEYS}
    for k in ('casts', 'missed', 'capped'):
        out[k] = np.array([int(r.get('report', {}).get(k, 0)) for r in results], dtype=np.int64)
    out.update(modes=results[0]['modes'], n=results[0]['n'], columns=len(results), report={})
    return out


def scaled_column(col, s):
    """A column flown with tau / s on the unscaled mesh as the structure scaled by s: lengths and times times s, squares s^2."""
    s = float(s)
    out = dict(col)
    out['D'] = np.asarray(col['D']) * s
    out['D2'] = np.asarray(col['D2']) * (s * s)
    out['T'] = np.asarray(col['T']) * s
    return out


def summarise_sweep(res, kind, values, omega, group_vel, taus, qv, T, axis=0, hbar=None, kb=None, points=200):
    """Per column what free_path.summarise returns, with `value` (the swept one) added: dict kind, values, axis, n, modes,
    columns (the list of summaries), grid and sampled [K, G], bulk [K, G] (the accumulation over the mean free path of every
    column on ONE common grid).  kind 'scale': column c is scaled_column(column c, s_c) with the lifetimes taus[c] s_c at the
    temperature T -- the structure scaled by s_c; 'temperature': column c with taus[c] and C_m at values[c] (T is ignored)."""
    if kind not in KINDS:
        raise ValueError('summarise_sweep: kind must be one of %s, got %r' % (', '.join(KINDS), kind))
    vals = np.asarray(values, dtype=np.float64).ravel()
    taus = np.asarray(taus, dtype=np.float64)
    cols = []
    for c, val in enumerate(vals):
        col = column(res, c)
        if kind == 'scale':
            s = FP.summarise(scaled_column(col, val), omega, group_vel, taus[c] * val, qv, T, axis=axis, hbar=hbar, kb=kb, points=points)
        else:
            s = FP.summarise(col, omega, group_vel, taus[c], qv, float(val), axis=axis, hbar=hbar, kb=kb, points=points)
        s['value'] = float(val)
        cols.append(s)
    grid = MD.accumulation_grid(np.concatenate([s['accumulation']['mfp'] for s in cols]) if cols else np.zeros(0), points, log=True)
    sampled = np.stack([MD.accumulation(s['k_mode'], s['accumulation']['mfp'], grid) for s in cols])
    bulk = np.stack([MD.accumulation(s['k_mode_bulk'], s['accumulation']['mfp'], grid) for s in cols])
    return dict(kind=kind, values=vals, axis=int(axis), n=int(res['n']), modes=np.asarray(res['modes'], dtype=np.int32), columns=cols,
                grid=grid, sampled=sampled, bulk=bulk, report=dict(res.get('report', {})))


# ------------------------------------------------------------------------------------------- files
def k_free_path_sweep_path(folder):
    return os.path.join(folder, 'k_free_path_sweep.txt')


def free_path_sweep_npz_path(folder):
    return os.path.join(folder, 'free_path_sweep.npz')


def write_k_free_path_sweep(path, sw):
    """k_free_path_sweep.txt from summarise_sweep(): one line per column -- the swept value, kappa along the axis (W/m K), its
    standard error, the bulk value, their ratio, rays missed, rays cut off, the largest w_left / n."""
    a = sw['axis']
    rows = [[s['value'], s['kappa'][a, a], s['kappa_se'][a, a], s['kappa_bulk'][a, a],
             s['kappa'][a, a] / s['kappa_bulk'][a, a] if s['kappa_bulk'][a, a] != 0 else np.nan, s['missed'], s['capped'], s['w_left_max']]
            for s in sw['columns']]
    header = ('free-path sweep: geometry-limited conductivity by ray casts, one set of casts weighed per column (an estimate in every '
              'column: exact where the walls that end the flights are parallel to the transport direction, an approximation where '
              'reservoirs end them along it)\nkind %s\nN %d\naxis %d\n%s kappa kappa_se kappa_bulk ratio missed capped w_left_max'
              % (sw['kind'], sw['n'], a, sw['kind']))
    np.savetxt(path, np.array(rows, dtype=np.float64).reshape(-1, 8), fmt='% .17e', header=header)
    return path


def read_k_free_path_sweep(path):
    """dict kind, N, axis, values, kappa, kappa_se, kappa_bulk, ratio, w_left_max [K] (floats), missed, capped [K] (ints)."""
    out = {}
    with open(path) as f:
        for line in f:
            if not line.startswith('#'):
                break
            w = line[1:].split()
            if len(w) == 2 and w[0] == 'kind':
                out['kind'] = w[1]
            elif len(w) == 2 and w[0] in ('N', 'axis'):
                out[w[0]] = int(w[1])
    d = np.loadtxt(path, ndmin=2)
    out.update(values=d[:, 0], kappa=d[:, 1], kappa_se=d[:, 2], kappa_bulk=d[:, 3], ratio=d[:, 4], missed=d[:, 5].astype(np.int64),
               capped=d[:, 6].astype(np.int64), w_left_max=d[:, 7])
    return out


def write_free_path_sweep_npz(path, sw):
    """free_path_sweep.npz: kind, values, n, axis, modes; per column the kappa tensors (kappa, kappa_se, kappa_bulk [K, 3, 3]),
    the per-mode suppression [K, L, 3] and the accumulation over the mean free path on the common grid (grid [G], cum_k_sampled,
    cum_k_bulk [K, G]), missed, capped, w_left_max [K]."""
    cols = sw['columns']
    st = lambda key, dt=np.float64: np.array([np.asarray(s[key]) for s in cols], dtype=dt)
    np.savez_compressed(path, kind=np.str_(sw['kind']), values=sw['values'], n=np.int64(sw['n']), axis=np.int64(sw['axis']), modes=sw['modes'],
                        kappa=st('kappa'), kappa_se=st('kappa_se'), kappa_bulk=st('kappa_bulk'), suppression=st('suppression'),
                        grid=sw['grid'], cum_k_sampled=sw['sampled'], cum_k_bulk=sw['bulk'], missed=st('missed', np.int64),
                        capped=st('capped', np.int64), w_left_max=st('w_left_max'))
    return path


def read_free_path_sweep_npz(path):
    with np.load(path) as z:
        out = {k: z[k] for k in z.files}
    out['kind'] = str(out['kind'])
    return out
