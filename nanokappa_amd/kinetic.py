"""Kinetic flights: the host side of Engine.kinetic_flights (nk_kinetic_flights, k_kinetic) -- NumPy only, usable without a GPU.

The engine solves the steady linearised BTE in the relaxation-time picture by the deviational, time-step-free Monte Carlo
(DESIGN.md "Kinetic flights"): energy packets leave the reservoirs ('T' facets), fly along their group velocity, scatter after an
exponential time into a mode drawn in proportion to c_m / tau_m, are re-emitted by diffuse walls and absorbed by reservoirs.
From the counts and the integer sums it returns this module forms

    the transmission T_fg = ends_fg / N and the conductance G_fg = g_f T_fg (W/K) with its binomial standard error,
    g_f = A_f sum_m c_m (v_m . n_f)+ the strength of source f (n_f its inward normal),
    for reservoir temperatures T_f, by superposition, the temperature deviation and the heat flux of every subvolume,
    and, between two parallel reservoirs of equal area A at distance L, kappa_eff = G_01 L / A.

Unlike the free-path estimate (free_path.py) this conserves energy: it is exact in the linear regime, also where reservoirs end
the flights along the transport direction.

Units are the package's: angstrom, ps, K, eV; conductances in W/K, conductivities in W/m K, heat fluxes in W/m^2."""
import math
import os

import numpy as np

from . import free_path as FP
from .constants import Constants
from .engine import KIN_ROW_CLAMPED

N_DEFAULT = 65536
MAX_EVENTS_DEFAULT = 2 ** 20
MAX_SOURCES = 8               # NK_KIN_MAX_SOURCES (include/nanokappa_hip.h)
TRIALS = 64                   # NK_KIN_TRIALS
END_LOST, END_MISSED, END_CAPPED = -1, -2, -3


def kinetic_option(value):
    """--kinetic N [T] [max_events] -> (N, T or None, max_events); N = 0: off (the option is absent, or given as 0).
    T (K) defaults to the mean reservoir temperature (None here), max_events to MAX_EVENTS_DEFAULT."""
    if value is None:
        return 0, None, MAX_EVENTS_DEFAULT
    v = list(value) if isinstance(value, (list, tuple)) else [value]
    if len(v) == 0:
        return 0, None, MAX_EVENTS_DEFAULT
    usage = '--kinetic: expected N [T] [max_events] (rays per source > 0, temperature in K > 0, events per ray > 0), got %r' % ' '.join(str(x) for x in v)
    if len(v) > 3:
        raise ValueError(usage)
    try:
        n = int(v[0])
        T = float(v[1]) if len(v) > 1 else None
        me = int(v[2]) if len(v) > 2 else MAX_EVENTS_DEFAULT
    except ValueError:
        raise ValueError(usage)
    if n == 0 and len(v) == 1:
        return 0, None, MAX_EVENTS_DEFAULT
    if n <= 0 or me <= 0 or (T is not None and not (T > 0 and np.isfinite(T))):
        raise ValueError(usage)
    return n, T, me


def watt():
    """eV / ps in W."""
    c = Constants()
    return c.eVpsa2_in_Wm2 * c.a_in_m * c.a_in_m


def heat_capacity(omega, T, qv, hbar=None, kb=None):
    """c_m [M]: the volumetric heat capacity per mode, hbar omega dn/dT / (Q V) (eV / K angstrom^3) -- free_path.kappa's constant."""
    return FP.mode_heat_capacity(np.ravel(omega), T, hbar, kb) / float(qv)


def live_modes(c, tau):
    """A mode is live when c_m > 0 and tau_m > 0; the others are never drawn."""
    return (np.ravel(c) > 0) & (np.ravel(tau) > 0)


def _cumulative(w):
    """A cumulative table that ends at 1, by a plain left-to-right sum (np.cumsum adds in order), so NumPy and the device see the
    same array."""
    w = np.asarray(w, dtype=np.float64)
    if not (np.all(np.isfinite(w)) and w.sum() > 0):
        raise ValueError('kinetic.tables: no live mode, or a weight that is not finite')
    cdf = np.cumsum(w)
    return cdf / cdf[-1]


def tables(c, tau, group_vel):
    """(cdf_scatter, cdf_flux) [M]: cumulative c_m / tau_m and c_m |v_m| over the live modes, each normalised to end at 1."""
    c, tau = np.ravel(np.asarray(c, dtype=np.float64)), np.ravel(np.asarray(tau, dtype=np.float64))
    v = np.asarray(group_vel, dtype=np.float64).reshape(-1, 3)
    if not (c.shape == tau.shape and v.shape[0] == c.shape[0]):
        raise ValueError('kinetic.tables: c, tau and group_vel must hold one entry per mode')
    lv = live_modes(c, tau)
    with np.errstate(divide='ignore', invalid='ignore'):
        ws = np.where(lv, c / np.where(lv, tau, 1.0), 0.0)
    speed = np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])
    return _cumulative(ws), _cumulative(np.where(lv, c * speed, 0.0))


def source_facets(bound_cond):
    """The sources: the facets with boundary condition 'T', ascending.  Refuses 'F' facets, no source, more than MAX_SOURCES."""
    bc = np.asarray(bound_cond)
    if bc.dtype.kind in 'US':
        bc = np.array([ord(str(x)[0]) for x in bc])
    bc = bc.astype(np.int64)
    if (bc == ord('F')).any():
        raise ValueError("kinetic flights: facet %d has boundary condition 'F' (a fixed heat flux): reservoirs 'T', periodic 'P' and rough 'R' "
                         "facets only" % int(np.nonzero(bc == ord('F'))[0][0]))
    src = np.nonzero(bc == ord('T'))[0]
    if src.size == 0:
        raise ValueError("kinetic flights: no facet with boundary condition 'T': nothing emits")
    if src.size > MAX_SOURCES:
        raise ValueError("kinetic flights: %d facets with boundary condition 'T' are more than the %d sources a call takes" % (src.size, MAX_SOURCES))
    return src.astype(np.int32)


def source_strength(area, normal_in, c, group_vel, live=None):
    """g_f = A_f sum_m c_m (v_m . n_f)+ (W/K), n_f the inward normal: summed exactly (math.fsum)."""
    c = np.ravel(np.asarray(c, dtype=np.float64))
    v = np.asarray(group_vel, dtype=np.float64).reshape(-1, 3)
    keep = np.ones(c.shape, dtype=bool) if live is None else np.ravel(live)
    out = []
    for A, n in zip(np.ravel(area), np.asarray(normal_in, dtype=np.float64).reshape(-1, 3)):
        vn = (v[:, 0] * n[0] + v[:, 1] * n[1]) + v[:, 2] * n[2]
        out.append(float(A) * math.fsum((c * np.maximum(vn, 0.0))[keep]) * watt())
    return np.array(out)


def transmission(ends, n):
    """T_fg = ends / N and its binomial standard error."""
    T = np.asarray(ends, dtype=np.float64) / float(n)
    return T, np.sqrt(np.maximum(T * (1.0 - T), 0.0) / float(n))


def profile(res, g, dT_f, sv_volume, c_total):
    """By superposition, for the sources' deviations dT_f (K) from the reference temperature: the temperature deviation of every
    subvolume dT_s = sum_f g_f dT_f dwell[f][s] / (N V_s sum_m c_m) (K) and its heat flux q_s [S, 3] = sum_f g_f dT_f flux[f][s] /
    (N V_s) (W/m^2).  g (W/K), sv_volume (angstrom^3), c_total = sum of c_m over the live modes (eV / K angstrom^3)."""
    w = np.asarray(g, dtype=np.float64) * np.asarray(dT_f, dtype=np.float64) / float(res['n'])            # W per ray
    V = np.asarray(sv_volume, dtype=np.float64)
    dT = np.einsum('f,fs->s', w, np.asarray(res['dwell'], dtype=np.float64)) / (V * float(c_total) * watt())
    a = Constants().a_in_m
    q = np.einsum('f,fsa->sa', w, np.asarray(res['flux'], dtype=np.float64)) / V[:, None] / (a * a)
    return dT, q


def parallel_pair(src_facets, normals, areas, centroids):
    """(L, A, axis) where exactly two sources are parallel planes of equal area facing each other, else None."""
    if len(src_facets) != 2:
        return None
    n0, n1 = np.asarray(normals[src_facets[0]], dtype=float), np.asarray(normals[src_facets[1]], dtype=float)
    A0, A1 = float(areas[src_facets[0]]), float(areas[src_facets[1]])
    if not (np.allclose(n0, -n1, atol=1e-9) and abs(A0 - A1) <= 1e-9 * max(A0, A1)):
        return None
    L = abs(float(np.dot(np.asarray(centroids[src_facets[1]], dtype=float) - np.asarray(centroids[src_facets[0]], dtype=float), n0)))
    if not L > 0:
        return None
    return L, A0, int(np.argmax(np.abs(n0)))


def derived(rows, sub, report, grp=None, map=None):
    """What a result holds besides n, the sources and the tables, from its integers rows [F, 32], sub [F, S, 4] (int64) and the
    report's scales k_*: the counts ends, lost, missed, capped, events, casts, the reals D, D2, dwell_total, dwell, flux (an integer
    times 2^-k: exact), and rows and sub themselves; with grp [F, S, G + 1, 4] also grp, dwell_g, flux_g; with map [F, nx, ny, nz,
    4] also map, dwell_map, flux_map and clamped.  Engine.kinetic_flights forms one call's result with it, kinetic_groups.pool and
    kinetic_map.pool the pooled one."""
    nf = rows.shape[0]
    st, sx = 2.0 ** -report['k_t'], 2.0 ** -report['k_x']
    out = dict(ends=rows[:, :nf].copy(), lost=rows[:, 8].copy(), missed=rows[:, 9].copy(), capped=rows[:, 10].copy(),
               events=rows[:, 11].copy(), casts=rows[:, 12].copy(), D=rows[:, 13:16] * 2.0 ** -report['k_D'],
               D2=rows[:, 16:19] * 2.0 ** -report['k_D2'], dwell_total=rows[:, 19] * 2.0 ** -report['k_T'], dwell=sub[:, :, 0] * st,
               flux=sub[:, :, 1:4] * sx, rows=rows, sub=sub)
    if grp is not None:
        out.update(grp=grp, dwell_g=grp[..., 0] * st, flux_g=grp[..., 1:4] * sx)
    if map is not None:
        out.update(map=map, dwell_map=map[..., 0] * st, flux_map=map[..., 1:4] * sx, clamped=rows[:, KIN_ROW_CLAMPED].copy())
    return out


def left_out(res):
    """(overflow, message) of an Engine.kinetic_flights result or of kinetic_groups.pool(): how many terms lay above their bounds
    and were left out of the integer sums (a call that leaves terms out still returns its results), and the engine's text."""
    rep = res.get('report', {}) or {}
    return int(rep.get('overflow', 0) or 0), str(rep.get('message', '') or '')


def left_out_warning(s):
    """The one line Population.kinetic_flights prints for a summarise() dict whose sums miss terms; None where none was left out."""
    if int(s.get('overflow', 0)) <= 0:
        return None
    return 'Warning: kinetic flights: %d term(s) above their bounds were left out of the sums: %s' % (
        int(s['overflow']), ' '.join(str(s.get('message', '')).split()) or 'the engine gave no text')


def summarise(res, c, group_vel, tau, T, areas, normals_in, T_f, sv_volume, pair=None, omega_c=None, qv=None):
    """Everything one reads off an Engine.kinetic_flights result.  areas [F], normals_in [F, 3] of the sources; T_f [F] their
    temperatures (T_ref = the mean); sv_volume [S]; pair: parallel_pair()'s (L, A, axis) or None.  `overflow` (int) and `message`
    are left_out()'s: above 0, terms are missing from the sums and every figure below is short of them.  With omega_c = C_m (eV / K, the
    per-mode heat capacity of free_path) and qv also the bulk conductivity and the free-path estimate's closed form along the axis."""
    n = int(res['n'])
    lv = live_modes(c, tau)
    g = source_strength(areas, normals_in, c, group_vel, lv)
    Tm, Tse = transmission(res['ends'], n)
    G, Gse = g[:, None] * Tm, g[:, None] * Tse
    T_f = np.asarray(T_f, dtype=np.float64)
    T_ref = float(T_f.mean())
    ct = math.fsum(np.ravel(c)[lv])
    dT, q = profile(res, g, T_f - T_ref, sv_volume, ct)
    out = dict(T=float(T), n=n, source_facet=np.asarray(res['source_facet'], dtype=np.int32), g=g, transmission=Tm, transmission_se=Tse,
               G=G, G_se=Gse, T_f=T_f, T_ref=T_ref, dT=dT, q=q, ends=np.asarray(res['ends'], dtype=np.int64),
               lost=np.asarray(res['lost'], dtype=np.int64), missed=np.asarray(res['missed'], dtype=np.int64),
               capped=np.asarray(res['capped'], dtype=np.int64), events=np.asarray(res['events'], dtype=np.int64),
               casts=np.asarray(res['casts'], dtype=np.int64), D=np.asarray(res['D']), D2=np.asarray(res['D2']),
               dwell_total=np.asarray(res['dwell_total']), dwell=np.asarray(res['dwell']), flux=np.asarray(res['flux']),
               report=dict(res.get('report', {})), overflow=left_out(res)[0], message=left_out(res)[1], kappa_eff=np.nan, kappa_eff_se=np.nan, kappa_bulk=np.nan, kappa_free_path=np.nan,
               L=np.nan, A=np.nan, axis=-1)
    if pair is not None:
        L, A, axis = pair
        a = Constants().a_in_m
        G01, G01se = 0.5 * (G[0, 1] + G[1, 0]), 0.5 * math.hypot(Gse[0, 1], Gse[1, 0])
        out.update(L=float(L), A=float(A), axis=int(axis), kappa_eff=G01 * L / A / a, kappa_eff_se=G01se * L / A / a)
        if omega_c is not None and qv is not None:
            v = np.asarray(group_vel, dtype=np.float64).reshape(-1, 3)
            t = np.where(lv, np.ravel(tau), 0.0)
            C = np.where(lv, np.ravel(omega_c), 0.0)
            out['kappa_bulk'] = float(FP.bulk_kappa(C, v, t, qv)[axis, axis])
            Dcf = np.zeros_like(v)
            Dcf[:, axis] = FP.film_displacement(v[:, axis], t, L)
            out['kappa_free_path'] = float(FP.kappa_tensor(C, v, Dcf, qv)[axis, axis])
    return out


# ------------------------------------------------------------------------------------------- files
def k_kinetic_path(folder):
    return os.path.join(folder, 'k_kinetic.txt')


def kinetic_npz_path(folder):
    return os.path.join(folder, 'kinetic.npz')


_SCALARS = ('T', 'T_ref', 'L', 'A', 'kappa_eff', 'kappa_eff_se', 'kappa_bulk', 'kappa_free_path')
_INTS = ('N', 'axis')
_ROWS = ('source_facet', 'g', 'T_f', 'lost', 'missed', 'capped', 'events', 'casts')


def write_k_kinetic(path, s):
    """k_kinetic.txt from summarise(): header lines (T, N, the sources, their strengths and temperatures, kappa_eff with its standard
    error where two parallel reservoirs define it, the bulk value and the free-path closed form, the counts), then the matrices G and
    G_se (W/K), one row per source: G_f0 .. G_fF-1 then G_se_f0 .. G_se_fF-1."""
    v = dict(s, N=s['n'])
    lines = ['kinetic flights: conductance between the reservoirs from the steady linearised BTE (relaxation time), exact in the linear regime']
    for k in _SCALARS:
        lines.append('%s %.17e' % (k, v[k]))
    for k in _INTS:
        lines.append('%s %d' % (k, v[k]))
    for k in _ROWS:
        a = np.ravel(v[k])
        lines.append(k + ' ' + ' '.join(('%d' % x) if a.dtype.kind in 'iu' else ('%.17e' % x) for x in a))
    lines.append('G[f][0..F-1] G_se[f][0..F-1]  (W/K)')
    np.savetxt(path, np.hstack([np.atleast_2d(s['G']), np.atleast_2d(s['G_se'])]), fmt='% .17e', header='\n'.join(lines))
    return path


def read_k_kinetic(path):
    """dict of a k_kinetic.txt: the header's scalars and rows, G and G_se [F, F]."""
    out = {}
    with open(path) as f:
        for line in f:
            if not line.startswith('#'):
                break
            w = line[1:].split()
            if len(w) < 2:
                continue
            if w[0] in _SCALARS and len(w) == 2:
                out[w[0]] = float(w[1])
            elif w[0] in _INTS and len(w) == 2:
                out[w[0]] = int(w[1])
            elif w[0] in _ROWS:
                out[w[0]] = np.array([float(x) for x in w[1:]]) if w[0] in ('g', 'T_f') else np.array([int(x) for x in w[1:]], dtype=np.int64)
    d = np.atleast_2d(np.loadtxt(path))
    F = d.shape[0]
    out.update(G=d[:, :F], G_se=d[:, F:2 * F])
    return out


def write_kinetic_npz(path, s):
    """kinetic.npz: the transmission, the per-subvolume dT and q, the sums and the report's numbers."""
    rep = {('report_' + k): np.asarray(v) for k, v in s['report'].items() if np.isscalar(v)}
    np.savez_compressed(path, **{k: np.asarray(s[k]) for k in ('T', 'n', 'source_facet', 'g', 'transmission', 'transmission_se', 'G', 'G_se',
                                                               'T_f', 'T_ref', 'dT', 'q', 'ends', 'lost', 'missed', 'capped', 'events', 'casts', 'D',
                                                               'D2', 'dwell_total', 'dwell', 'flux', 'kappa_eff', 'kappa_eff_se', 'kappa_bulk',
                                                               'kappa_free_path', 'L', 'A', 'axis')}, **rep)
    return path


def read_kinetic_npz(path):
    with np.load(path) as z:
        return {k: z[k] for k in z.files}
