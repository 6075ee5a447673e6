"""Kinetic maps: the host side of Engine.kinetic_flights(..., grid=) (nk_kinetic_flights_map, k_kinetic<., ., false, true>) -- NumPy
only, usable without a GPU.

In a map call every segment of the kinetic flights (kinetic.py) that adds its four integers {t 2^k_t, t v_a 2^k_x} to the words of
(source, subvolume of x_p) adds the same four integers to the line of (source, cell of x_p) on the field's grid (field.py: cell =
floor((x - lo) * (1 / h)) per axis, an index outside clamped into the edge cell and counted).  x_p is the one uniform point of the
segment, so for every source and word the cells add up to the subvolumes bit for bit (DESIGN.md "Kinetic maps").  From the map this
module forms, by kinetic.profile's superposition with the cells in the place of the subvolumes, the steady temperature deviation dT
(K), T = T_ref + dT and the heat flux q (W/m^2) of every cell, with standard errors from the spread over batches of flights.

Here: the option parser, the pooling of batches, summarise_map, and the writers / readers of kinetic_map.npz and kinetic_map.vtk.

Units are the package's: angstrom, ps, K, eV; heat fluxes in W/m^2."""
import math
import os

import numpy as np

from . import field as FD
from . import kinetic as KN
from . import kinetic_groups as KG

VOLUMES = ('cell', 'solid')
BATCHES_DEFAULT = 8           # what --kinetic_map uses: the error bars are the spread over the batches
MAX_MAP_WORDS = 1 << 27       # NK_KIN_MAX_MAP_WORDS (include/nanokappa_hip.h)


def kinetic_map_option(value, kinetic_n=None):
    """--kinetic_map nx ny nz [cell|solid] -> ((nx, ny, nz), volume), or (None, 'cell') when off (the option is absent, or
    0 0 0).  kinetic_n: the N of --kinetic where the caller knows it; the map needs it (> 0)."""
    v = list(value) if isinstance(value, (list, tuple)) else ([] if value is None else [value])
    usage = '--kinetic_map: expected nx ny nz [cell|solid] (positive cell counts, at most 2^24 cells), got %r' % ' '.join(str(x) for x in v)
    if not v:
        return None, 'cell'
    if len(v) not in (3, 4):
        raise ValueError(usage)
    try:
        n = tuple(int(x) for x in v[:3])
    except ValueError:
        raise ValueError(usage)
    volume = str(v[3]) if len(v) == 4 else 'cell'
    if volume not in VOLUMES:
        raise ValueError(usage)
    if n == (0, 0, 0):
        return None, volume
    if min(n) <= 0 or n[0] * n[1] * n[2] > FD.MAX_CELLS:
        raise ValueError(usage)
    if kinetic_n is not None and int(kinetic_n) <= 0:
        raise ValueError('--kinetic_map requires --kinetic N [T] [max_events]: the map bins the segments of the kinetic flights')
    return n, volume


# ------------------------------------------------------------------------------------------------ batches
def pool(results):
    """The pooled result of B map calls with the same n, max_events, lifetimes and grid under different seeds:
    kinetic_groups.pool's sums of rows and sub, and the elementwise integer sum of map (with dwell_map, flux_map and clamped)."""
    out = KG.pool(results)
    first = results[0]
    if 'map' in first:
        for r in results[1:]:
            if np.shape(r['map']) != np.shape(first['map']):
                raise ValueError('kinetic_map.pool: the calls differ in their grid')
        m = sum(np.asarray(r['map'], dtype=np.int64) for r in results)
        out.update(KN.derived(out['rows'], out['sub'], out['report'], map=m))
    return out


# ------------------------------------------------------------------------------------------------ the superposition per cell
def cell_profile(res, g, dT_f, volume, c_total):
    """(dT [ncells], q [ncells, 3]) of one result through kinetic.profile: the map's dwell and flux as [F, ncells]."""
    dw = np.asarray(res['dwell_map'], dtype=np.float64)
    F = dw.shape[0]
    with np.errstate(divide='ignore', invalid='ignore'):
        return KN.profile(dict(n=res['n'], dwell=dw.reshape(F, -1), flux=np.asarray(res['flux_map'], dtype=np.float64).reshape(F, -1, 3)),
                          g, dT_f, np.ravel(volume), c_total)


def summarise_map(res, c, group_vel, tau, areas, normals_in, T_f, lo, h, n_cells, volume='cell', solid_volume=None, batches=None):
    """Per cell of the grid (lo, h, n_cells) the steady temperature deviation dT (K), T = T_ref + dT and the heat flux q [.., 3]
    (W/m^2) of an Engine.kinetic_flights(..., grid=) result (or of pool()): kinetic.profile with the cells in the subvolumes'
    place.  areas [F], normals_in [F, 3], T_f [F] of the sources (T_ref = the mean), as kinetic.summarise.  volume 'cell': a cell's
    volume is h_x h_y h_z; 'solid': solid_volume [nx, ny, nz] (Engine-side cell_solid_volume), which also gives solid_fraction.  A
    cell whose dwell word is 0 for every source, or whose solid fraction is 0, is NaN.  batches: the B results that were pooled
    into res -- every standard error (dT_se = T_se, q_se) is std(ddof = 1) / sqrt(B) of the batches' own cell quantities, NaN
    for B = 1 or without batches."""
    if volume not in VOLUMES:
        raise ValueError('summarise_map: volume must be one of %s, got %r' % (', '.join(VOLUMES), volume))
    nc = tuple(int(k) for k in n_cells)
    lo, h = np.asarray(lo, dtype=np.float64).reshape(3), np.asarray(h, dtype=np.float64).reshape(3)
    m = np.asarray(res['map'], dtype=np.int64)
    if m.shape[1:] != nc + (4,):
        raise ValueError('summarise_map: the map has the shape %r, the grid %r cells' % (m.shape, nc))
    cell = float(h[0] * h[1] * h[2])
    fraction = None
    if volume == 'solid':
        if solid_volume is None:
            raise ValueError("summarise_map: volume 'solid' needs solid_volume (the solid volume of every cell)")
        V = np.asarray(solid_volume, dtype=np.float64).reshape(nc)
        fraction = V / cell
    else:
        V = np.full(nc, cell)
    lv = KN.live_modes(c, tau)
    g = KN.source_strength(areas, normals_in, c, group_vel, lv)
    T_f = np.asarray(T_f, dtype=np.float64)
    T_ref = float(T_f.mean())
    ct = math.fsum(np.ravel(c)[lv])
    empty = (m[..., 0] == 0).all(axis=0) | ~(V > 0)

    def one(r):
        dT, q = cell_profile(r, g, T_f - T_ref, V, ct)
        dT, q = dT.reshape(nc), q.reshape(nc + (3,))
        return np.where(empty, np.nan, dT), np.where(empty[..., None], np.nan, q)
    dT, q = one(res)
    per = list(batches) if batches is not None else []
    if len(per) > 1:
        bd, bq = zip(*(one(r) for r in per))
        dT_se, q_se = KG.mean_se(bd)[1], KG.mean_se(bq)[1]
        dT_se, q_se = np.where(empty, np.nan, dT_se), np.where(empty[..., None], np.nan, q_se)
    else:
        dT_se, q_se = np.full(nc, np.nan), np.full(nc + (3,), np.nan)
    out = dict(lo=lo, h=h, n=nc, volume=volume, n_samples=int(res['n']), batches=max(len(per), 1), T_ref=T_ref, T_f=T_f, g=g,
               source_facet=np.asarray(res['source_facet'], dtype=np.int32), dT=dT, dT_se=dT_se, T=T_ref + dT, T_se=dT_se, q=q, q_se=q_se,
               map=m, clamped=np.asarray(res['clamped'], dtype=np.int64), cell_volume=V, report=dict(res.get('report', {})),
               overflow=KN.left_out(res)[0])
    if fraction is not None:
        out['solid_fraction'] = fraction
    return out


# ------------------------------------------------------------------------------------------------ files
def kinetic_map_npz_path(folder):
    return os.path.join(folder, 'kinetic_map.npz')


def kinetic_map_vtk_path(folder):
    return os.path.join(folder, 'kinetic_map.vtk')


_ARRAYS = ('dT', 'dT_se', 'T', 'T_se', 'q', 'q_se', 'map', 'clamped', 'cell_volume', 'solid_fraction', 'T_f', 'g', 'source_facet')
_INTS = ('n_samples', 'batches', 'overflow')


def write_kinetic_map_npz(path, s):
    """kinetic_map.npz from summarise_map(): every array, the grid, the integers of the map and the report's numbers."""
    out = {k: np.asarray(s[k]) for k in _ARRAYS if s.get(k) is not None}
    out.update(lo=np.asarray(s['lo'], dtype=np.float64), h=np.asarray(s['h'], dtype=np.float64), n=np.asarray(s['n'], dtype=np.int64),
               volume=np.array(s['volume']), T_ref=np.float64(s['T_ref']))
    for k in _INTS:
        out[k] = np.int64(s[k])
    for k, v in s.get('report', {}).items():
        if np.isscalar(v) and not isinstance(v, str):
            out['report_' + k] = np.asarray(v)
    np.savez_compressed(path, **out)
    return path


def read_kinetic_map_npz(path):
    """What write_kinetic_map_npz wrote, with the report as a dict again."""
    with np.load(path) as z:
        raw = {k: z[k] for k in z.files}
    out, rep = {}, {}
    for k, v in raw.items():
        if k.startswith('report_'):
            rep[k[7:]] = v.item()
        elif k == 'volume':
            out[k] = str(v)
        elif k in _INTS:
            out[k] = int(v)
        elif k == 'T_ref':
            out[k] = float(v)
        elif k == 'n':
            out[k] = tuple(int(x) for x in v)
        else:
            out[k] = v
    out['report'] = rep
    return out


def vtk_title(s, T=None):
    """The title line of kinetic_map.vtk: what was flown and how many segment points were clamped into the grid's edge cells."""
    return 'nanokappa kinetic map: steady T and q%s, %d rays per source in %d batches, volume %s, %d points clamped' % (
        '' if T is None else ' at T = %g K' % T, int(s['n_samples']), int(s['batches']), s['volume'], int(np.sum(s['clamped'])))


def write_kinetic_map_vtk(path, s, title=None):
    """Legacy ASCII VTK in field.write_vtk's layout and cell order (it can be laid beside field.vtk): scalars T, dT, T_se, dT_se and,
    where known, solid_fraction; vectors q and q_se.  The title line carries the points clamped."""
    n = tuple(int(k) for k in s['n'])
    scalars = [('T', s['T']), ('dT', s['dT']), ('T_se', s['T_se']), ('dT_se', s['dT_se'])]
    if s.get('solid_fraction') is not None:
        scalars.append(('solid_fraction', np.asarray(s['solid_fraction'], dtype=np.float64).reshape(n)))
    with open(path, 'w') as f:
        f.write('# vtk DataFile Version 3.0\n%s\nASCII\nDATASET STRUCTURED_POINTS\n' % (title or vtk_title(s)).replace('\n', ' ')[:255])
        f.write('DIMENSIONS %d %d %d\n' % (n[0] + 1, n[1] + 1, n[2] + 1))
        f.write('ORIGIN %.17g %.17g %.17g\n' % tuple(np.asarray(s['lo'], dtype=float)))
        f.write('SPACING %.17g %.17g %.17g\n' % tuple(np.asarray(s['h'], dtype=float)))
        f.write('CELL_DATA %d\n' % (n[0] * n[1] * n[2]))
        for name, arr in scalars:
            f.write('SCALARS %s double 1\nLOOKUP_TABLE default\n' % name)
            f.write('\n'.join('%.17g' % x for x in FD._vtk_order(np.asarray(arr, dtype=np.float64).reshape(n))) + '\n')
        for name, arr in (('q', s['q']), ('q_se', s['q_se'])):
            f.write('VECTORS %s double\n' % name)
            f.write('\n'.join('%.17g %.17g %.17g' % tuple(r) for r in FD._vtk_order(np.asarray(arr, dtype=np.float64).reshape(n + (3,)))) + '\n')
    return path


def read_kinetic_map_vtk(path):
    """What write_kinetic_map_vtk wrote (field.read_vtk reads the layout): dict lo, h, n, title, T, dT, T_se, dT_se (nx, ny, nz), q,
    q_se (nx, ny, nz, 3) and solid_fraction where the file holds it."""
    return FD.read_vtk(path)
