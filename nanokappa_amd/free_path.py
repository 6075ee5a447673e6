"""Free-path sampling: the host side of Engine.free_paths (nk_free_paths, k_free_paths) -- NumPy only, usable without a GPU.

The engine flies n rays per mode from start points uniform in the solid along the mode's group velocity until a boundary ends
them, weighs every segment with the intrinsic lifetime and returns per-mode sums: the displacement D, its squares, the flight
time, the weights that ended at reservoirs, at diffuse walls and intrinsically.  From those this module forms

    kappa_ab = 1 / (Q V) sum_m C_m v_{m,a} mean(D_{m,b}),      C_m = hbar omega_m dn/dT at T,

its standard error (from the squares), the bulk value (mean(D) = v tau), the suppression of every mode, the closed form for
walls normal to the transport axis at distance L (box T T P), and the conductivity accumulated over the mean free path.

An ESTIMATE: exact (Fuchs-Sondheimer) where the walls that end the flights are parallel to the transport direction (films,
wires along their axis); an approximation where reservoirs end the flights along it.

Units are the package's: angstrom, ps, K, eV; conductivities in W/m K."""
import os

import numpy as np

from . import modes as MD
from .constants import Constants

N_DEFAULT = 64
MAX_SEGMENTS_DEFAULT = 65536
W_MIN_DEFAULT = 2.0 ** -40
END_CODES = ('weight exhausted', 'reservoir', 'diffuse wall', 'miss', 'cap')


def free_path_option(value):
    """--free_path N [T] [max_segments] -> (N, T or None, max_segments); N = 0: off (the option is absent, or given as 0).
    T (K) defaults to the mean reservoir temperature (None here), max_segments to MAX_SEGMENTS_DEFAULT."""
    if value is None:
        return 0, None, MAX_SEGMENTS_DEFAULT
    v = list(value) if isinstance(value, (list, tuple)) else [value]
    if len(v) == 0:
        return 0, None, MAX_SEGMENTS_DEFAULT
    usage = '--free_path: expected N [T] [max_segments] (rays per mode > 0, temperature in K > 0, casts per ray > 0), got %r' % ' '.join(str(x) for x in v)
    if len(v) > 3:
        raise ValueError(usage)
    try:
        n = int(v[0])
        T = float(v[1]) if len(v) > 1 else None
        ms = int(v[2]) if len(v) > 2 else MAX_SEGMENTS_DEFAULT
    except ValueError:
        raise ValueError(usage)
    if n == 0 and len(v) == 1:
        return 0, None, MAX_SEGMENTS_DEFAULT
    if n <= 0 or ms <= 0 or (T is not None and not (T > 0 and np.isfinite(T))):
        raise ValueError(usage)
    return n, T, ms


def default_modes(group_vel, tau):
    """The default list: every mode with |v| > 0 and tau > 0 (global indices q*J + j)."""
    v = np.asarray(group_vel, dtype=np.float64).reshape(-1, 3)
    t = np.asarray(tau, dtype=np.float64).ravel()
    return np.nonzero((np.abs(v).max(axis=1) > 0) & (t > 0))[0].astype(np.int32)


def lifetimes(phonon, T):
    """tau [M] of every mode at temperature T: Phonon.lifetime_function, T clipped into the table."""
    Q, J = phonon.omega.shape
    g = phonon.temperature_array
    q, j = np.meshgrid(np.arange(Q), np.arange(J), indexing='ij')
    Tqj = np.stack([np.full(Q * J, float(np.clip(T, g[0], g[-1]))), q.ravel(), j.ravel()], axis=1)
    return np.asarray(phonon.lifetime_function(Tqj), dtype=np.float64).ravel()


def mode_heat_capacity(omega, T, hbar=None, kb=None):
    """C_m = hbar omega dn/dT at T (eV / K) = kb x^2 e^x / (e^x - 1)^2, x = hbar omega / (kb T); 0 where omega <= 0."""
    c = Constants()
    hbar = c.hbar if hbar is None else float(hbar)
    kb = c.kb if kb is None else float(kb)
    om = np.asarray(omega, dtype=np.float64)
    x = np.where(om > 0, hbar * om / (kb * float(T)), 1.0)
    em1 = np.expm1(x)
    with np.errstate(over='ignore', invalid='ignore'):
        cm = kb * x * x * (em1 + 1.0) / (em1 * em1)
    return np.where((om > 0) & np.isfinite(cm), cm, 0.0)


def _unit():
    c = Constants()
    return c.eVpsa2_in_Wm2 * c.a_in_m           # eV / (ps angstrom K) -> W / (m K)


def mean_displacement(res):
    """mean(D) [L, 3] and the variance of that mean [L, 3] (from the squares; n - 1 in the denominator) of a free_paths result."""
    n = float(res['n'])
    D = np.asarray(res['D'], dtype=np.float64) / n
    var = np.maximum(np.asarray(res['D2'], dtype=np.float64) / n - D * D, 0.0) / max(n - 1.0, 1.0)
    return D, var


def kappa_tensor(C, group_vel, Dbar, qv, var=None):
    """kappa [3, 3] (W/m K) = 1 / (Q V) sum_m C_m v_{m,a} Dbar_{m,b}; with var [L, 3] (the variance of every Dbar) also its
    standard error [3, 3].  C [L], group_vel [L, 3], Dbar [L, 3]: the modes of the list."""
    C = np.asarray(C, dtype=np.float64).ravel()
    v = np.asarray(group_vel, dtype=np.float64).reshape(-1, 3)
    D = np.asarray(Dbar, dtype=np.float64).reshape(-1, 3)
    w = C[:, None] * v                                                   # [L, 3]
    k = _unit() / float(qv) * np.einsum('ma,mb->ab', w, D)
    if var is None:
        return k
    se = _unit() / float(qv) * np.sqrt(np.einsum('ma,mb->ab', w * w, np.asarray(var, dtype=np.float64).reshape(-1, 3)))
    return k, se


def bulk_kappa(C, group_vel, tau, qv):
    """The bulk tensor: kappa_tensor with Dbar = v tau."""
    v = np.asarray(group_vel, dtype=np.float64).reshape(-1, 3)
    return kappa_tensor(C, v, v * np.asarray(tau, dtype=np.float64).ravel()[:, None], qv)


def suppression(Dbar, group_vel, tau):
    """Dbar_a / (v_a tau) per mode and axis [L, 3]; NaN where v_a tau = 0."""
    v = np.asarray(group_vel, dtype=np.float64).reshape(-1, 3)
    vt = v * np.asarray(tau, dtype=np.float64).ravel()[:, None]
    with np.errstate(divide='ignore', invalid='ignore'):
        return np.where(vt != 0, np.asarray(Dbar, dtype=np.float64).reshape(-1, 3) / vt, np.nan)


def film_suppression(mfp_x, L):
    """1 - (Lambda / L) (1 - exp(-L / Lambda)) for Lambda = |v_x| tau: the expectation of D_x / (v_x tau) over start points uniform
    between two absorbing (or diffuse) walls normal to x at distance L, everything else periodic.  1 for Lambda = 0."""
    lam = np.abs(np.asarray(mfp_x, dtype=np.float64))
    with np.errstate(divide='ignore', invalid='ignore'):
        s = 1.0 + (lam / float(L)) * np.expm1(-float(L) / lam)
    return np.where(lam > 0, s, 1.0)


def film_displacement(vx, tau, L):
    """The closed form's mean displacement v_x tau [1 - (Lambda_x / L)(1 - exp(-L / Lambda_x))]; 0 for v_x = 0."""
    vx = np.asarray(vx, dtype=np.float64)
    tau = np.asarray(tau, dtype=np.float64)
    return vx * tau * film_suppression(vx * tau, L)


def mode_kappa(C, group_vel, Dbar, qv, axis=0):
    """Every mode's share of kappa_aa along `axis` [L] (W/m K)."""
    v = np.asarray(group_vel, dtype=np.float64).reshape(-1, 3)
    return _unit() / float(qv) * np.asarray(C, dtype=np.float64).ravel() * v[:, axis] * np.asarray(Dbar, dtype=np.float64).reshape(-1, 3)[:, axis]


def accumulation(C, group_vel, tau, Dbar, qv, axis=0, points=200):
    """Conductivity along `axis` accumulated over the mean free path |v| tau (modes.accumulation on modes.accumulation_grid):
    dict grid [G], bulk [G], sampled [G] (cumulative, the last point = the total), mfp [L]."""
    v = np.asarray(group_vel, dtype=np.float64).reshape(-1, 3)
    t = np.asarray(tau, dtype=np.float64).ravel()
    mfp = np.linalg.norm(v, axis=1) * t
    grid = MD.accumulation_grid(mfp, points, log=True)
    kb = mode_kappa(C, v, v * t[:, None], qv, axis)
    ks = mode_kappa(C, v, Dbar, qv, axis)
    return dict(grid=grid, bulk=MD.accumulation(kb, mfp, grid), sampled=MD.accumulation(ks, mfp, grid), mfp=mfp)


def summarise(res, omega, group_vel, tau, qv, T, axis=0, hbar=None, kb=None, points=200):
    """Everything one reads off an Engine.free_paths result: dict T, n, modes, tau, C, D_mean, D_var, kappa, kappa_se, kappa_bulk
    [3, 3], suppression [L, 3], k_mode, k_mode_bulk [L] (along `axis`), accumulation (dict), missed, capped, w_left_max (the
    largest w_left / n), invariant (the largest |p_res + p_wall + w_left + p_int - n| / n), report.  omega, group_vel, tau: the
    material's tables over ALL modes; the result's list picks from them."""
    ml = np.asarray(res['modes'], dtype=np.int64)
    om = np.asarray(omega, dtype=np.float64).ravel()[ml]
    v = np.asarray(group_vel, dtype=np.float64).reshape(-1, 3)[ml]
    t = np.asarray(tau, dtype=np.float64).ravel()[ml]
    C = mode_heat_capacity(om, T, hbar, kb)
    D, var = mean_displacement(res)
    k, se = kappa_tensor(C, v, D, qv, var)
    n = float(res['n'])
    inv = np.abs(res['p_res'] + res['p_wall'] + res['w_left'] + res['p_int'] - n) / n
    rep = dict(res.get('report', {}))
    return dict(T=float(T), n=int(res['n']), axis=int(axis), modes=ml.astype(np.int32), tau=t, C=C, D_mean=D, D_var=var, kappa=k,
                kappa_se=se, kappa_bulk=bulk_kappa(C, v, t, qv), suppression=suppression(D, v, t),
                k_mode=mode_kappa(C, v, D, qv, axis), k_mode_bulk=mode_kappa(C, v, v * t[:, None], qv, axis),
                accumulation=accumulation(C, v, t, D, qv, axis, points), missed=int(rep.get('missed', 0)),
                capped=int(rep.get('capped', 0)), w_left_max=float(np.max(res['w_left'] / n)) if ml.size else 0.0,
                invariant=float(inv.max()) if ml.size else 0.0, report=rep,
                sums={key: np.asarray(res[key]) for key in ('D', 'D2', 'T', 'hits', 'p_res', 'p_wall', 'w_left', 'p_int')})


# ------------------------------------------------------------------------------------------- files
def k_free_path_path(folder):
    return os.path.join(folder, 'k_free_path.txt')


def free_path_npz_path(folder):
    return os.path.join(folder, 'free_path.npz')


def _row(a):
    return ' '.join('%.17e' % x for x in np.ravel(a))


def write_k_free_path(path, s):
    """k_free_path.txt from summarise(): header lines T, N, the kappa tensor and its standard error, the bulk tensor, missed,
    capped and the largest w_left / n; then one line per grid point: mean free path (angstrom), cumulative bulk kappa and
    cumulative sampled kappa along the axis (W/m K)."""
    a = s['accumulation']
    header = ('free-path sampling: geometry-limited conductivity by ray casts (an estimate: exact where the walls that end the flights '
              'are parallel to the transport direction, an approximation where reservoirs end them along it)\n'
              'T %.17e\nN %d\naxis %d\nkappa %s\nkappa_se %s\nkappa_bulk %s\nmissed %d\ncapped %d\nw_left_max %.17e\n'
              'mean_free_path cum_k_bulk cum_k_sampled' % (s['T'], s['n'], s['axis'], _row(s['kappa']), _row(s['kappa_se']), _row(s['kappa_bulk']),
                                                             s['missed'], s['capped'], s['w_left_max']))
    np.savetxt(path, np.column_stack([a['grid'], a['bulk'], a['sampled']]), fmt='% .17e', header=header)
    return path


def read_k_free_path(path):
    """dict T, N, axis, kappa, kappa_se, kappa_bulk [3, 3], missed, capped, w_left_max, grid, bulk, sampled of a k_free_path.txt."""
    out = {}
    with open(path) as f:
        for line in f:
            if not line.startswith('#'):
                break
            w = line[1:].split()
            if not w:
                continue
            if w[0] in ('kappa', 'kappa_se', 'kappa_bulk') and len(w) == 10:
                out[w[0]] = np.array([float(x) for x in w[1:]]).reshape(3, 3)
            elif w[0] in ('T', 'w_left_max') and len(w) == 2:
                out[w[0]] = float(w[1])
            elif w[0] in ('N', 'axis', 'missed', 'capped') and len(w) == 2:
                out[w[0]] = int(w[1])
    d = np.atleast_2d(np.loadtxt(path))
    out.update(grid=d[:, 0], bulk=d[:, 1], sampled=d[:, 2])
    return out


def write_free_path_npz(path, s):
    """free_path.npz: the per-mode arrays of summarise() (modes, tau, C, the sums, D_mean, D_var, suppression, k_mode,
    k_mode_bulk) and the scalars T, n, axis, kappa, kappa_se, kappa_bulk, missed, capped."""
    np.savez_compressed(path, T=np.float64(s['T']), n=np.int64(s['n']), axis=np.int64(s['axis']), modes=s['modes'], tau=s['tau'], C=s['C'],
                        D_mean=s['D_mean'], D_var=s['D_var'], suppression=s['suppression'], k_mode=s['k_mode'], k_mode_bulk=s['k_mode_bulk'],
                        kappa=s['kappa'], kappa_se=s['kappa_se'], kappa_bulk=s['kappa_bulk'], missed=np.int64(s['missed']),
                        capped=np.int64(s['capped']), **{'sum_' + k: v for k, v in s['sums'].items()})
    return path


def read_free_path_npz(path):
    with np.load(path) as z:
        return {k: z[k] for k in z.files}
