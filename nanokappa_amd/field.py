"""Spatial field maps: particle count N, deviational energy E = sum e_i and heat flux F = sum v_i e_i on a uniform grid over
the geometry's bounding box -- the GPU-native counterpart of the reference's particle scatter plots (--fig_plot / --colormap,
Population.plot_figures, reference classes/Population.py:1841-1979).  The engine sums them (Engine.set_field, k_field); this
module is the host side, NumPy only and usable without a GPU: the grid, a float64 restatement of the sums (what the tests hold
the GPU against), the reference's normalisations per cell, and a VTK writer / reader.

Grid convention (the engine's, include/nanokappa_hip.h nk_field): cell of a particle = floor((x - lo) * (1 / h)) per axis, an
index outside [0, n) clamped into the edge cell (and counted in `clamped`); arrays are shaped (nx, ny, nz[, 3])."""
import numpy as np

FIELD_EVERY_DEFAULT = 100          # the reference's plotting cadence (Population.py:1735)
MAX_CELLS = 1 << 24


def field_grid_option(value):
    """--field_grid nx ny nz [every] -> ((nx, ny, nz), every) or (None, every) when off (no value, or 0 0 0)."""
    v = list(value or [])
    usage = '--field_grid: expected nx ny nz [every] (positive cell counts, every > 0), got %r' % ' '.join(str(x) for x in v)
    if not v:
        return None, FIELD_EVERY_DEFAULT
    if len(v) not in (3, 4):
        raise ValueError(usage)
    try:
        iv = [int(x) for x in v]
    except ValueError:
        raise ValueError(usage)
    n, every = tuple(iv[:3]), (iv[3] if len(iv) == 4 else FIELD_EVERY_DEFAULT)
    if n == (0, 0, 0):
        return None, every
    if min(n) <= 0 or every <= 0 or n[0] * n[1] * n[2] > MAX_CELLS:
        raise ValueError(usage)
    return n, every


def grid_from_bounds(bounds, n):
    """(lo, h, n) of the grid of n = (nx, ny, nz) cells that spans bounds = [[lo], [hi]] (Geometry.bounds)."""
    b = np.asarray(bounds, dtype=np.float64).reshape(2, 3)
    n = np.asarray(n, dtype=np.int64).reshape(3)
    if np.any(n <= 0) or np.any(b[1] <= b[0]):
        raise ValueError('grid_from_bounds: needs positive cell counts and a box of positive extent')
    return b[0].copy(), (b[1] - b[0]) / n, tuple(int(k) for k in n)


def cell_index(pos, lo, h, n):
    """Cell (ix, iy, iz) [N, 3] of every position, clamped into the grid, and the mask of the positions that were clamped."""
    pos = np.asarray(pos, dtype=np.float64).reshape(-1, 3)
    lo, h = np.asarray(lo, dtype=np.float64), np.asarray(h, dtype=np.float64)
    nn = np.asarray(n, dtype=np.int64)
    f = np.floor((pos - lo) * (1.0 / h))
    out = ~((f >= 0) & (f < nn))                         # (a NaN coordinate counts as outside: edge cell 0)
    c = np.where(f >= 0, np.minimum(f, nn - 1), 0)
    c = np.where(np.isnan(f), 0, c).astype(np.int64)
    return c, out.any(axis=1)


def cell_centres(lo, h, n):
    """Centres of all cells, [nx, ny, nz, 3]."""
    ax = [np.asarray(lo, dtype=float)[a] + (np.arange(n[a]) + 0.5) * np.asarray(h, dtype=float)[a] for a in range(3)]
    return np.stack(np.meshgrid(*ax, indexing='ij'), axis=-1)


def _flat(c, n):
    return (c[:, 0] * n[1] + c[:, 1]) * n[2] + c[:, 2]


def field_from_particles(pos, e, v, lo, h, n):
    """The sums in float64: dict N (nx, ny, nz), E, F (.., 3), clamped.  pos [P, 3], e [P], v [P, 3]."""
    n = tuple(int(k) for k in n)
    c, out = cell_index(pos, lo, h, n)
    q = _flat(c, n)
    nc = n[0] * n[1] * n[2]
    e = np.asarray(e, dtype=np.float64).ravel()
    v = np.asarray(v, dtype=np.float64).reshape(-1, 3)
    N = np.bincount(q, minlength=nc).astype(np.float64)
    E = np.bincount(q, weights=e, minlength=nc)
    F = np.stack([np.bincount(q, weights=v[:, a] * e, minlength=nc) for a in range(3)], axis=-1)
    return dict(N=N.reshape(n), E=E.reshape(n), F=F.reshape(n + (3,)), clamped=int(out.sum()))


def quantised(pos, e, v, lo, h, n, k_E, k_F):
    """The same sums the way the GPU forms them: every term scaled by 2^k, rounded to nearest (rint) and added as int64.
    dict raw (nx, ny, nz, 8) int64 = {N, E 2^k_E, Fx 2^k_F, Fy 2^k_F, Fz 2^k_F, 0, 0, 0}, N, E, F (the reals they stand for),
    clamped.  Equal to the engine's integers bit for bit whenever the host's terms e, v e equal the device's; per cell they
    differ from the float64 sums by at most n_cell 2^-(k + 1)."""
    n = tuple(int(k) for k in n)
    c, out = cell_index(pos, lo, h, n)
    q = _flat(c, n)
    nc = n[0] * n[1] * n[2]
    e = np.asarray(e, dtype=np.float64).ravel()
    v = np.asarray(v, dtype=np.float64).reshape(-1, 3)
    raw = np.zeros((nc, 8), dtype=np.int64)
    np.add.at(raw[:, 0], q, 1)
    np.add.at(raw[:, 1], q, np.rint(np.ldexp(e, int(k_E))).astype(np.int64))
    for a in range(3):
        np.add.at(raw[:, 2 + a], q, np.rint(np.ldexp(v[:, a] * e, int(k_F))).astype(np.int64))
    return dict(raw=raw.reshape(n + (8,)), N=raw[:, 0].astype(np.float64).reshape(n),
                E=np.ldexp(raw[:, 1].astype(np.float64), -int(k_E)).reshape(n),
                F=np.ldexp(raw[:, 2:5].astype(np.float64), -int(k_F)).reshape(n + (3,)), clamped=int(out.sum()))


def normalise(N, E, F, samples, active_modes, QV, eVpsa2_in_Wm2, norm='mean', particle_density=None, cell_volume=None,
              ref_energy=None, temperature_function=None):
    """The reference's scalings, per cell, of sums over `samples` field steps.
    energy density (eV/angstrom^3): E * active_modes / N ('mean', --energy_normal mean; the ratio of the window's sums) or
      (E / samples) * active_modes / (particle_density * cell_volume) ('fixed'), through normalise_to_density (/ QV, QV =
      number_of_qpoints * volume_unitcell), plus ref_energy (Population.py:719-728): the reference energy of the subvolume the
      cell's CENTRE lies in (a cell that straddles two subvolumes takes its centre's), an array shaped like N or None;
    T: temperature_function(energy) -- the material's T(E) table; None when no function is given;
    heat_flux (W/m^2): F with the same scaling, times eVpsa2_in_Wm2 (Population.py:738-747).
    For 'fixed', cell_volume is the WHOLE cell's volume, so cells cut by the surface of the solid read low (the exact solid
    fraction of cut cells is not computed).  Cells with N = 0 give NaN.  Returns dict N (mean count per sample), energy, T,
    heat_flux."""
    N = np.asarray(N, dtype=np.float64)
    E = np.asarray(E, dtype=np.float64)
    F = np.asarray(F, dtype=np.float64)
    s = max(int(samples), 1)
    with np.errstate(divide='ignore', invalid='ignore'):
        if norm == 'fixed':
            if particle_density is None or cell_volume is None:
                raise ValueError("normalise: 'fixed' needs particle_density and cell_volume")
            scale = np.where(N > 0, active_modes / (particle_density * cell_volume * s), np.nan)
        elif norm == 'mean':
            scale = np.where(N > 0, active_modes / N, np.nan)
        else:
            raise ValueError('normalise: norm must be mean or fixed')
        energy = E * scale / QV
        flux = F * scale[..., None] / QV * eVpsa2_in_Wm2
    if ref_energy is not None:
        energy = energy + np.asarray(ref_energy, dtype=np.float64)
    T = None
    if temperature_function is not None:
        T = np.full(energy.shape, np.nan)
        ok = ~np.isnan(energy)
        if ok.any():
            T[ok] = np.asarray(temperature_function(energy[ok]), dtype=np.float64)
    return dict(N=N / s, energy=energy, T=T, heat_flux=flux)


# ------------------------------------------------------------------------------------------------ VTK
def _vtk_order(a):
    """(nx, ny, nz[, k]) -> rows in VTK's cell order (x fastest)."""
    a = np.asarray(a, dtype=np.float64)
    return a.transpose(2, 1, 0).reshape(-1) if a.ndim == 3 else a.transpose(2, 1, 0, 3).reshape(-1, a.shape[3])


def write_vtk(path, lo, h, n, N, T, energy, heat_flux, title='nanokappa field'):
    """Legacy ASCII VTK, STRUCTURED_POINTS with CELL_DATA: scalars N, T, energy and the vector heat_flux (any viewer opens it;
    full float64 precision, NaN where a cell is empty)."""
    n = tuple(int(k) for k in n)
    nc = n[0] * n[1] * n[2]
    T = np.full(n, np.nan) if T is None else T
    with open(path, 'w') as f:
        f.write('# vtk DataFile Version 3.0\n%s\nASCII\nDATASET STRUCTURED_POINTS\n' % title.replace('\n', ' ')[:255])
        f.write('DIMENSIONS %d %d %d\n' % (n[0] + 1, n[1] + 1, n[2] + 1))
        f.write('ORIGIN %.17g %.17g %.17g\n' % tuple(np.asarray(lo, dtype=float)))
        f.write('SPACING %.17g %.17g %.17g\n' % tuple(np.asarray(h, dtype=float)))
        f.write('CELL_DATA %d\n' % nc)
        for name, a in (('N', N), ('T', T), ('energy', energy)):
            f.write('SCALARS %s double 1\nLOOKUP_TABLE default\n' % name)
            f.write('\n'.join('%.17g' % x for x in _vtk_order(a)) + '\n')
        f.write('VECTORS heat_flux double\n')
        f.write('\n'.join('%.17g %.17g %.17g' % tuple(r) for r in _vtk_order(heat_flux)) + '\n')
    return path


def read_vtk(path):
    """What write_vtk wrote: dict lo, h, n, title, N, T, energy (nx, ny, nz), heat_flux (nx, ny, nz, 3)."""
    with open(path) as f:
        lines = f.read().split('\n')
    if not lines[0].startswith('# vtk') or lines[2].strip() != 'ASCII' or lines[3].split() != ['DATASET', 'STRUCTURED_POINTS']:
        raise ValueError('read_vtk: %s is not a legacy ASCII STRUCTURED_POINTS file' % path)
    out = dict(title=lines[1])
    i = 4
    n = None
    while i < len(lines):
        w = lines[i].split()
        i += 1
        if not w:
            continue
        if w[0] == 'DIMENSIONS':
            n = tuple(int(x) - 1 for x in w[1:4])
            out['n'] = n
        elif w[0] == 'ORIGIN':
            out['lo'] = np.array([float(x) for x in w[1:4]])
        elif w[0] == 'SPACING':
            out['h'] = np.array([float(x) for x in w[1:4]])
        elif w[0] == 'CELL_DATA':
            nc = int(w[1])
            if n is None or nc != n[0] * n[1] * n[2]:
                raise ValueError('read_vtk: CELL_DATA does not match DIMENSIONS')
        elif w[0] == 'SCALARS':
            i += 1                                           # LOOKUP_TABLE
            a = np.array([float(x) for x in lines[i:i + nc]])
            i += nc
            out[w[1]] = a.reshape(n[2], n[1], n[0]).transpose(2, 1, 0).copy()
        elif w[0] == 'VECTORS':
            a = np.array([[float(x) for x in r.split()] for r in lines[i:i + nc]])
            i += nc
            out[w[1]] = a.reshape(n[2], n[1], n[0], 3).transpose(2, 1, 0, 3).copy()
    return out


def field_path(folder):
    import os
    return os.path.join(folder, 'field.vtk')
