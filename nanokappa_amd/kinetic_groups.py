"""Kinetic groups: the kinetic flights' per-subvolume sums split by group of modes -- which phonons carry the heat between the
reservoirs and how far the groups are out of equilibrium with each other.  A group is a frequency bin, a branch, a mean-free-path
bin, a direction bin (field_groups.py's vocabulary) or any table of the caller's.  The engine tallies them
(Engine.kinetic_flights(groups=...), nk_kinetic_flights_groups, k_kinetic<GEOM, BINS, true>); this module is the host side, NumPy
only and usable without a GPU: the option, the tables, the pooling of batches, the superposition per group and the files
k_kinetic_groups.txt and kinetic_groups.npz.

A table [Q*J] holds the group 0 .. G-1 of every mode or -1; the engine returns G + 1 columns, the last one -- the REST column --
for the modes with -1 (live modes that do not move have no mean free path and no direction), so that the columns always add up
to the ungrouped words `sub`, as integers, bit for bit.

Conventions and units are kinetic.profile's: angstrom, ps, K, eV; heat fluxes in W/m^2, conductivities in W/m K."""
import math
import os

import numpy as np

from . import field_groups as FG
from . import free_path as FP
from . import kinetic as KN
from .constants import Constants

KINDS = FG.KINDS
MAX_GROUPS = 256              # NK_KIN_MAX_GROUPS (include/nanokappa_hip.h)
BATCHES_DEFAULT = 8           # what --kinetic_groups uses: the error bars are the spread over the batches


def kinetic_groups_option(value, kinetic_n=None):
    """--kinetic_groups G kind [axis] -> (G, kind, axis); (0, None, None) when off (no value, or G = 0).  field_groups_option's
    rules: kind one of frequency, branch, mfp, direction; axis (x, y, z or 0, 1, 2; direction only) is None where the transport
    axis is meant.  With kinetic_n (the N of --kinetic) given, the option is refused where --kinetic is off."""
    v = list(value or [])
    usage = ('--kinetic_groups: expected G kind [axis] (0 < G <= %d groups; kind one of %s; axis x, y or z, for direction), got %r'
             % (MAX_GROUPS, ', '.join(KINDS), ' '.join(str(x) for x in v)))
    if not v:
        return 0, None, None
    try:
        G = int(v[0])
    except ValueError:
        raise ValueError(usage)
    if G == 0 and len(v) == 1:
        return 0, None, None
    if len(v) not in (2, 3) or G <= 0 or G > MAX_GROUPS:
        raise ValueError(usage)
    kind = str(v[1])
    if kind not in KINDS:
        raise ValueError(usage)
    axis = None
    if len(v) == 3:
        if kind != 'direction' or str(v[2]).lower() not in FG._AXES:
            raise ValueError(usage)
        axis = FG._AXES[str(v[2]).lower()]
    if kinetic_n is not None and int(kinetic_n) <= 0:
        raise ValueError('--kinetic_groups requires --kinetic N [T] [max_events]: the groups are tallied by the kinetic flights')
    return G, kind, axis


# ------------------------------------------------------------------------------------------------ tables
def build(kind, G, phonon, tau, group_vel, axis=0):
    """(group_of_mode int32 [Q*J], G, edges) through field_groups' builders.  'mfp' bins |v_m| tau_m of the CALL's lifetimes `tau`
    [Q*J] (not the material's at some temperature: a caller may pass its own); a mode with tau <= 0 or v = 0 gets -1.  'branch'
    takes G from the material."""
    inactive = getattr(phonon, 'inactive_modes_mask', None)
    if kind == 'frequency':
        return FG.frequency_groups(phonon.omega, G, inactive)
    if kind == 'branch':
        return FG.branch_groups(phonon.omega, inactive)
    if kind == 'mfp':
        v = np.asarray(group_vel, dtype=np.float64).reshape(-1, 3)
        t = np.asarray(tau, dtype=np.float64).ravel()
        if t.shape[0] != v.shape[0]:
            raise ValueError('kinetic_groups.build: tau has %d entries, the material %d modes' % (t.shape[0], v.shape[0]))
        speed = np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])
        return FG.mfp_groups(np.where(t > 0, speed * np.where(t > 0, t, 0.0), 0.0), G, inactive)
    if kind == 'direction':
        return FG.direction_groups(group_vel, G, 0 if axis is None else axis, inactive)
    raise ValueError('unknown group kind %r (%s)' % (kind, ', '.join(KINDS)))


def check_table(table, G, M=None):
    """The table as int32 [M] with entries in -1 .. G-1, 0 < G <= MAX_GROUPS; ValueError with the cause otherwise."""
    G = int(G)
    if not 0 < G <= MAX_GROUPS:
        raise ValueError('kinetic groups: n_groups = %d must be 1 .. %d' % (G, MAX_GROUPS))
    if table is None:
        raise ValueError('kinetic groups: the table is None (the group of every mode)')
    t = np.ascontiguousarray(np.ravel(table), dtype=np.int32)
    if M is not None and t.shape[0] != int(M):
        raise ValueError('kinetic groups: the table has %d entries, the material %d modes' % (t.shape[0], int(M)))
    return t


def columns(table, G):
    """The column of every mode: its group, or G (the rest column) where the table holds -1."""
    t = np.asarray(table, dtype=np.int64).ravel()
    return np.where(t < 0, int(G), t)


# ------------------------------------------------------------------------------------------------ batches
def pool(results):
    """The pooled result of B calls with the same n, max_events and lifetimes under different seeds: the elementwise sum of the
    integers rows, sub (and grp), N = B n, and everything Engine.kinetic_flights derives from them (the scales are the calls')."""
    first = results[0]
    rep = dict(first['report'])
    for r in results[1:]:
        for k in ('k_D', 'k_D2', 'k_T', 'k_t', 'k_x', 'n_sources', 'n_subvolumes'):
            if r['report'][k] != rep[k]:
                raise ValueError('kinetic_groups.pool: the calls differ in %s' % k)
        if r['n'] != first['n']:
            raise ValueError('kinetic_groups.pool: the calls differ in n')
    rows = sum(np.asarray(r['rows'], dtype=np.int64) for r in results)
    sub = sum(np.asarray(r['sub'], dtype=np.int64) for r in results)
    grp = sum(np.asarray(r['grp'], dtype=np.int64) for r in results) if 'grp' in first else None
    for k in ('rays', 'events', 'casts', 'lost', 'missed', 'capped', 'overflow', 'seconds', 'calls'):
        if k in rep:
            rep[k] = sum(r['report'][k] for r in results) if k != 'calls' else results[-1]['report'][k]
    rep['message'] = '; '.join(m for m in (KN.left_out(r)[1] for r in results) if m)      # (every call that left terms out says so)
    return dict(n=int(first['n']) * len(results), source_facet=np.asarray(first['source_facet']), **KN.derived(rows, sub, rep, grp=grp),
                cdf_scatter=first['cdf_scatter'], cdf_flux=first['cdf_flux'], report=rep, batches=len(results))


def mean_se(a):
    """(mean, std(ddof=1) / sqrt(B)) over the first axis; the standard error is NaN for B = 1."""
    a = np.asarray(a, dtype=np.float64)
    B = a.shape[0]
    with np.errstate(invalid='ignore', divide='ignore'):
        se = a.std(axis=0, ddof=1) / math.sqrt(B) if B > 1 else np.full(a.shape[1:], np.nan)
    return a.mean(axis=0), se


# ------------------------------------------------------------------------------------------------ the superposition per group
def group_heat_capacity(c, tau, table, G):
    """c_g [G + 1]: the sum of c_m over the live modes of every column (math.fsum)."""
    c = np.ravel(np.asarray(c, dtype=np.float64))
    lv = KN.live_modes(c, tau)
    col = columns(table, G)
    return np.array([math.fsum(c[lv & (col == g)]) for g in range(int(G) + 1)])


def profile_groups(res, g, dT_f, sv_volume, c_g):
    """kinetic.profile per column: dT_{s,g} = sum_f g_f dT_f dwell_g[f][s][g] / (N V_s c_g) (K; NaN where c_g = 0) and
    q_{s,g} [S, G + 1, 3] = sum_f g_f dT_f flux_g[f][s][g] / (N V_s) (W/m^2)."""
    w = np.asarray(g, dtype=np.float64) * np.asarray(dT_f, dtype=np.float64) / float(res['n'])
    V = np.asarray(sv_volume, dtype=np.float64)
    cg = np.asarray(c_g, dtype=np.float64)
    with np.errstate(divide='ignore', invalid='ignore'):
        dT = np.einsum('f,fsg->sg', w, np.asarray(res['dwell_g'], dtype=np.float64)) / (V[:, None] * np.where(cg > 0, cg, np.nan)[None, :] * KN.watt())
    a = Constants().a_in_m
    q = np.einsum('f,fsga->sga', w, np.asarray(res['flux_g'], dtype=np.float64)) / V[:, None, None] / (a * a)
    return dT, q


def flux_kappa(q, sv_volume, L, dT, sign=1.0):
    """L / dT times the volume average of q (W/m^2; the subvolumes on the first axis): W/m K.  L in angstrom; sign +1 where
    source 0 emits along +axis."""
    V = np.asarray(sv_volume, dtype=np.float64)
    q = np.asarray(q, dtype=np.float64)
    avg = np.tensordot(V, q, axes=(0, 0)) / V.sum()
    with np.errstate(divide='ignore', invalid='ignore'):
        return float(sign) * avg * (float(L) * Constants().a_in_m) / float(dT) if dT != 0 else avg * np.nan


def _quantities(res, g, T_f, sv_volume, c_g, pair, sign):
    dT, q = profile_groups(res, g, T_f - T_f.mean(), sv_volume, c_g)
    out = dict(dT_g=dT, q_g=q)
    if pair is not None:
        L, _, axis = pair
        k = flux_kappa(q[:, :, axis], sv_volume, L, T_f[0] - T_f[1], sign)
        out.update(kappa_g=k, kappa_flux=np.asarray(k.sum()), accumulation=np.cumsum(k[:-1]))
    return out


def summarise_groups(res, c, group_vel, tau, areas, normals_in, T_f, sv_volume, table, G, pair=None, omega_c=None, qv=None, kind=None,
                     edges=None, batches=None):
    """Everything one reads off a grouped Engine.kinetic_flights result (or pool() of several), by superposition for the sources'
    temperatures T_f [F] (T_ref = their mean): per column dT_g [S, G + 1] and q_g [S, G + 1, 3]; with pair = parallel_pair()'s
    (L, A, axis) also kappa_g [G + 1] = L / (T_0 - T_1) x the volume average of q_axis,g, their sum kappa_flux (the flux-based
    counterpart of kinetic.summarise's count-based kappa_eff), and the running sum over the G groups `accumulation` [G] (the
    accumulation function for 'mfp' and 'frequency'); with omega_c = C_m (eV / K) and qv also kappa_bulk_g (free_path.bulk_kappa
    on the column's live modes) and suppression = kappa_g / kappa_bulk_g.  batches: the B results that were pooled; every
    quantity q then has q_se = std(ddof=1) / sqrt(B) over them (NaN for B < 2 or without batches)."""
    G = int(G)
    table = check_table(table, G, np.ravel(c).shape[0])
    if np.asarray(res['grp']).shape[2] != G + 1:
        raise ValueError('summarise_groups: the result has %d columns, the table %d groups and the rest' % (np.asarray(res['grp']).shape[2], G))
    lv = KN.live_modes(c, tau)
    g = KN.source_strength(areas, normals_in, c, group_vel, lv)
    T_f = np.asarray(T_f, dtype=np.float64)
    c_g = group_heat_capacity(c, tau, table, G)
    V = np.asarray(sv_volume, dtype=np.float64)
    sign = 1.0
    if pair is not None:
        sign = 1.0 if np.asarray(normals_in, dtype=np.float64).reshape(-1, 3)[0][pair[2]] > 0 else -1.0
    out = dict(n=int(res['n']), G=G, kind='' if kind is None else str(kind), table=table,
               edges=np.asarray(edges if edges is not None else np.arange(G + 1) - 0.5, dtype=np.float64), c_g=c_g, g=g, T_f=T_f,
               T_ref=float(T_f.mean()), grp=np.asarray(res['grp'], dtype=np.int64), dwell_g=np.asarray(res['dwell_g']),
               flux_g=np.asarray(res['flux_g']), batches=0 if batches is None else len(batches), L=np.nan, A=np.nan, axis=-1,
               kappa_g=np.full(G + 1, np.nan), kappa_flux=np.asarray(np.nan), accumulation=np.full(G, np.nan),
               kappa_bulk_g=np.full(G + 1, np.nan), suppression=np.full(G + 1, np.nan), overflow=KN.left_out(res)[0],
               message=KN.left_out(res)[1])
    out.update(_quantities(res, g, T_f, V, c_g, pair, sign))
    if pair is not None:
        out.update(L=float(pair[0]), A=float(pair[1]), axis=int(pair[2]))
        if omega_c is not None and qv is not None:
            v = np.asarray(group_vel, dtype=np.float64).reshape(-1, 3)
            col = columns(table, G)
            t = np.where(lv, np.ravel(tau), 0.0)
            C = np.where(lv, np.ravel(omega_c), 0.0)
            out['kappa_bulk_g'] = np.array([float(FP.bulk_kappa(np.where(col == k, C, 0.0), v, t, qv)[pair[2], pair[2]]) for k in range(G + 1)])
    per = [_quantities(b, g, T_f, V, c_g, pair, sign) for b in (batches or [])]
    for k in ('dT_g', 'q_g', 'kappa_g', 'kappa_flux', 'accumulation'):
        if per and k in per[0]:
            out[k + '_se'] = mean_se([p[k] for p in per])[1]
        else:
            out[k + '_se'] = np.full(np.shape(out[k]), np.nan)
    with np.errstate(divide='ignore', invalid='ignore'):
        kb = np.where(out['kappa_bulk_g'] != 0, out['kappa_bulk_g'], np.nan)
        out['suppression'], out['suppression_se'] = out['kappa_g'] / kb, out['kappa_g_se'] / np.abs(kb)
    return out


# ------------------------------------------------------------------------------------------------ files
def k_kinetic_groups_path(folder):
    return os.path.join(folder, 'k_kinetic_groups.txt')


def kinetic_groups_npz_path(folder):
    return os.path.join(folder, 'kinetic_groups.npz')


_SCALARS = ('T_ref', 'L', 'A', 'kappa_flux', 'kappa_flux_se', 'kappa_rest', 'kappa_rest_se')
_INTS = ('N', 'G', 'axis', 'batches')
_COLS = ('edge_lo', 'edge_hi', 'kappa_g', 'kappa_g_se', 'kappa_bulk_g', 'suppression', 'accumulation')


def _edges_of(s):
    e = np.asarray(s['edges'], dtype=np.float64).ravel()
    G = int(s['G'])
    if e.shape[0] == G + 1:
        return e[:-1], e[1:]
    return np.arange(G) - 0.5, np.arange(G) + 0.5


def write_k_kinetic_groups(path, s):
    """k_kinetic_groups.txt from summarise_groups(): header lines (the kind, N, G, the axis, the batches, kappa_flux = the sum over
    all columns with its standard error, the rest column's share), then one line per group: its edges (frequency in rad/ps, mean
    free path in angstrom, cosine, or the index -+ 1/2), kappa_g and its standard error, kappa_bulk_g, the suppression, and the
    running sum of kappa_g (W/m K)."""
    G = int(s['G'])
    v = dict(s, N=s['n'], kappa_flux=float(s['kappa_flux']), kappa_flux_se=float(s['kappa_flux_se']), kappa_rest=float(s['kappa_g'][G]),
             kappa_rest_se=float(s['kappa_g_se'][G]))
    lines = ['kinetic groups: the conductivity between the reservoirs by group of modes, from the heat flux of the kinetic flights',
             'kind %s' % (s['kind'] or 'table')]
    for k in _SCALARS:
        lines.append('%s %.17e' % (k, v[k]))
    for k in _INTS:
        lines.append('%s %d' % (k, v[k]))
    lines.append(' '.join(_COLS) + '  (W/m K)')
    lo, hi = _edges_of(s)
    d = np.column_stack([lo, hi, s['kappa_g'][:G], s['kappa_g_se'][:G], s['kappa_bulk_g'][:G], s['suppression'][:G], s['accumulation']])
    np.savetxt(path, d, fmt='% .17e', header='\n'.join(lines))
    return path


def read_k_kinetic_groups(path):
    """dict of a k_kinetic_groups.txt: the header's entries and the columns [G] by name."""
    out = {}
    with open(path) as f:
        for line in f:
            if not line.startswith('#'):
                break
            w = line[1:].split()
            if len(w) != 2:
                continue
            if w[0] in _SCALARS:
                out[w[0]] = float(w[1])
            elif w[0] in _INTS:
                out[w[0]] = int(w[1])
            elif w[0] == 'kind':
                out['kind'] = w[1]
    d = np.atleast_2d(np.loadtxt(path))
    for i, k in enumerate(_COLS):
        out[k] = d[:, i]
    return out


_NPZ = ('n', 'G', 'kind', 'table', 'edges', 'c_g', 'g', 'T_f', 'T_ref', 'grp', 'dwell_g', 'flux_g', 'batches', 'L', 'A', 'axis', 'dT_g',
        'dT_g_se', 'q_g', 'q_g_se', 'kappa_g', 'kappa_g_se', 'kappa_flux', 'kappa_flux_se', 'accumulation', 'accumulation_se',
        'kappa_bulk_g', 'suppression', 'suppression_se')


def write_kinetic_groups_npz(path, s):
    """kinetic_groups.npz: the table and its edges, the integers grp [F, S, G + 1, 4], and every array of summarise_groups()."""
    np.savez_compressed(path, **{k: np.asarray(s[k]) for k in _NPZ})
    return path


def read_kinetic_groups_npz(path):
    with np.load(path) as z:
        out = {k: z[k] for k in z.files}
    out['kind'] = str(out['kind'])
    for k in ('n', 'G', 'batches', 'axis'):
        out[k] = int(out[k])
    return out
