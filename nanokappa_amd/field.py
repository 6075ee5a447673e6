"""Spatial field maps: particle count N, deviational energy E = sum e_i and heat flux F = sum v_i e_i on a uniform grid over
the geometry's bounding box -- the GPU-native counterpart of the reference's particle scatter plots (--fig_plot / --colormap,
Population.plot_figures, reference classes/Population.py:1841-1979).  The engine sums them (Engine.set_field, k_field); this
module is the host side, NumPy only and usable without a GPU: the grid, a float64 restatement of the sums (what the tests hold
the GPU against), the reference's normalisations per cell, the exact solid fraction of every cell (solid_volume, the restatement
of Engine-side nk_cell_solid_volume), and a VTK writer / reader.

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


def field_solid_option(value, field_n):
    """--field_solid -> bool; it needs --field_grid: the fractions are those of the field's cells."""
    on = bool(value)
    if on and field_n is None:
        raise ValueError('--field_solid requires --field_grid nx ny nz [every]: the solid fractions are those of the field\'s cells')
    return on


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


def mask_empty_volume(scale, cell_volume, shape):
    """`scale` with NaN where an array cell_volume is not positive; a scalar cell_volume leaves it as it is."""
    if np.ndim(cell_volume) == 0:
        return scale
    return np.where(np.asarray(cell_volume, dtype=np.float64) > 0, scale, np.nan)


def check_cell_volume(cell_volume, shape):
    """A cell volume is a number or an array shaped like the cells."""
    if np.ndim(cell_volume) != 0 and np.shape(cell_volume) != tuple(shape):
        raise ValueError('normalise: an array cell_volume must be shaped like the cells, %r, not %r' % (tuple(shape), np.shape(cell_volume)))


def normalise(N, E, F, samples, active_modes, QV, eVpsa2_in_Wm2, norm='mean', particle_density=None, cell_volume=None,
              ref_energy=None, temperature_function=None):
    """The reference's scalings, per cell, of sums over `samples` field steps.
    energy density (eV/angstrom^3): E * active_modes / N ('mean', --energy_normal mean; the ratio of the window's sums) or
      (E / samples) * active_modes / (particle_density * cell_volume) ('fixed'), through normalise_to_density (/ QV, QV =
      number_of_qpoints * volume_unitcell), plus ref_energy (Population.py:719-728): the reference energy of the subvolume the
      cell's CENTRE lies in (a cell that straddles two subvolumes takes its centre's), an array shaped like N or None;
    T: temperature_function(energy) -- the material's T(E) table; None when no function is given;
    heat_flux (W/m^2): F with the same scaling, times eVpsa2_in_Wm2 (Population.py:738-747).
    For 'fixed', cell_volume is a number -- the WHOLE cell's volume, so cells cut by the surface of the solid read low by their
    solid fraction -- or an array shaped like N with the volume of solid in every cell (solid_volume below, or
    Engine.cell_solid_volume: fraction x cell volume), which makes cut cells read right; a cell of zero volume gives NaN.
    Cells with N = 0 give NaN.  Returns dict N (mean count per sample), energy, T, heat_flux."""
    N = np.asarray(N, dtype=np.float64)
    E = np.asarray(E, dtype=np.float64)
    F = np.asarray(F, dtype=np.float64)
    s = max(int(samples), 1)
    with np.errstate(divide='ignore', invalid='ignore'):
        if norm == 'fixed':
            if particle_density is None or cell_volume is None:
                raise ValueError("normalise: 'fixed' needs particle_density and cell_volume")
            check_cell_volume(cell_volume, N.shape)
            scale = np.where(N > 0, active_modes / (particle_density * cell_volume * s), np.nan)
            scale = mask_empty_volume(scale, cell_volume, N.shape)
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


# ------------------------------------------------------------------------------------------------ solid fraction of the cells
# V[c] = volume of solid in cell c, exact for a closed triangle mesh with outward normals (no sampling): integrate the length of
# solid along x over the cell's (y, z) square.  A ray along x leaves the solid through faces with n_x > 0 and enters through
# faces with n_x < 0, so the length inside the cell's x slab [x_lo, x_lo + h_x] is the sum over the crossings of
# +-(x - x_lo) for a crossing in the slab, +-h_x for one beyond it, 0 for one before it.  Per triangle and cell, with the
# triangle clipped to the cell (Sutherland-Hodgman, closed slabs, order y_lo, y_hi, z_lo, z_hi, x_lo, x_hi):
#   a = signed area of the clipped polygon's projection on the yz plane (positive where n_x > 0),
#   p = integral of (x - x_lo) dy dz over the projection: x is linear on the polygon, so per fan triangle (vertex 0, i, i + 1)
#       it is a_i times (x_0 + x_i + x_{i+1}) / 3 - x_lo, exactly;
#   A[c] += a, P[c] += p, and V[ix] = P[ix] + h_x sum_{ix' > ix} A[ix'] (an exclusive suffix sum along x per (iy, iz) column).
# Everything is done in GRID UNITS u = (x - lo) / h per axis, so a cell is the unit cube [i, i + 1]^3, |a| <= 1, |p| <= 1, and V
# comes out in cells until the last multiplication by h_x h_y h_z.  That is what makes the ownership rule consistent: a
# triangle is offered to the cells floor(u) of its bounding box, clamped into [0, n), and clipped against the integers i and
# i + 1 -- the same numbers floor() compares with.  So a face lying IN a grid plane perpendicular to x (u = i for all three
# vertices) is offered to cell i alone, where it has x - x_lo = 0 and counts through A for the cells before it; a face in the
# grid's upper x boundary (u = n) lands in the last cell with x - x_lo = 1.  A vertex up to SOLID_SNAP cells outside the grid
# (the rounding of (x - lo) / h for a grid made from the mesh's own bounds) is moved onto the boundary; anything further out
# is an error: the grid must contain the mesh.
SOLID_SNAP = 1e-9
# a cell whose solid fraction is at most this counts as outside the solid: there the terms of entering and leaving faces cancel
# to rounding (a few 1e-16), not always to an exact 0
SOLID_EMPTY = 1e-12
_SOLID_CHUNK = 1 << 16          # (triangle, cell) pairs clipped at a time


def solid_grid_coordinates(vertices, faces, lo, h, n):
    """The triangles in grid units, [F, 3, 3], snapped into [0, n]; ValueError where the grid does not contain the mesh."""
    lo = np.asarray(lo, dtype=np.float64).reshape(3)
    h = np.asarray(h, dtype=np.float64).reshape(3)
    nn = np.asarray(n, dtype=np.int64).reshape(3)
    v = np.asarray(vertices, dtype=np.float64).reshape(-1, 3)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    if f.shape[0] <= 0:
        raise ValueError('solid_volume: no triangles')
    if np.any(nn <= 0) or int(nn[0]) * int(nn[1]) * int(nn[2]) > MAX_CELLS:
        raise ValueError('solid_volume: the grid needs 1 .. 2^24 cells')
    if not np.all(h > 0) or not np.all(np.isfinite(h)) or not np.all(np.isfinite(lo)):
        raise ValueError('solid_volume: the cell sizes h must be positive')
    u = (v[f] - lo) / h
    if not np.all((u >= -SOLID_SNAP) & (u <= nn + SOLID_SNAP)):               # (false for a NaN as well)
        raise ValueError('solid_volume: the grid does not contain the bounding box of the triangles')
    return np.minimum(np.maximum(u, 0.0), nn.astype(np.float64))


def _clip(poly, cnt, axis, bound, lower):
    """One Sutherland-Hodgman step for many polygons at once: poly [P, m, 3], cnt [P] vertices in use, against coordinate
    `axis` >= bound [P] (lower) or <= bound (upper), the plane itself inside.  -> (poly [P, m + 1, 3], cnt)."""
    P, m = poly.shape[0], poly.shape[1]
    idx = np.arange(m)[None, :]
    valid = idx < cnt[:, None]
    nxt_i = np.where(valid, (idx + 1) % np.maximum(cnt, 1)[:, None], 0)
    nxt = np.take_along_axis(poly, nxt_i[:, :, None], axis=1)
    b = bound[:, None]
    dc = poly[:, :, axis] - b if lower else b - poly[:, :, axis]
    dn = nxt[:, :, axis] - b if lower else b - nxt[:, :, axis]
    in_c, in_n = dc >= 0.0, dn >= 0.0
    with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
        t = dc / (dc - dn)
        inter = poly + t[:, :, None] * (nxt - poly)
    inter[:, :, axis] = np.broadcast_to(b, (P, m))
    out = np.empty((P, 2 * m, 3))
    out[:, 0::2], out[:, 1::2] = poly, inter
    keep = np.zeros((P, 2 * m), dtype=bool)
    keep[:, 0::2], keep[:, 1::2] = valid & in_c, valid & (in_c != in_n)
    order = np.argsort(~keep, axis=1, kind='stable')[:, :m + 1]
    return np.take_along_axis(out, order[:, :, None], axis=1), keep.sum(axis=1)


def solid_terms(u, cell):
    """(a, p) of triangles u [P, 3, 3] (grid units) clipped to the unit cells `cell` [P, 3] (integers): see above."""
    poly, cnt = np.array(u, dtype=np.float64), np.full(u.shape[0], 3, dtype=np.int64)
    c = np.asarray(cell, dtype=np.float64)
    for axis in (1, 2, 0):
        poly, cnt = _clip(poly, cnt, axis, c[:, axis], True)
        poly, cnt = _clip(poly, cnt, axis, c[:, axis] + 1.0, False)
    a = np.zeros(u.shape[0])
    p = np.zeros(u.shape[0])
    x0, y0, z0 = poly[:, 0, 0], poly[:, 0, 1], poly[:, 0, 2]
    for i in range(1, poly.shape[1] - 1):
        use = cnt > i + 1
        if not use.any():
            break
        with np.errstate(invalid='ignore', over='ignore'):      # (slots beyond cnt hold whatever the clips left there)
            ai = 0.5 * ((poly[:, i, 1] - y0) * (poly[:, i + 1, 2] - z0) - (poly[:, i + 1, 1] - y0) * (poly[:, i, 2] - z0))
            pi = ai * ((x0 + poly[:, i, 0] + poly[:, i + 1, 0]) / 3.0 - c[:, 0])
        a = a + np.where(use, ai, 0.0)
        p = p + np.where(use, pi, 0.0)
    return a, p


def solid_volume(vertices, faces, lo, h, n):
    """Volume of solid in every cell of the grid, (nx, ny, nz) float64, for a closed triangle mesh whose faces are wound so
    that their normals point out of the solid (mesh.Mesh's are): exact for the triangles, see the rule above.  The float64
    restatement of nk_cell_solid_volume (Engine.cell_solid_volume), which the tests hold the GPU against."""
    n = tuple(int(k) for k in np.asarray(n).reshape(3))
    u = solid_grid_coordinates(vertices, faces, lo, h, n)
    nn = np.asarray(n, dtype=np.int64)
    i0 = np.minimum(np.floor(u.min(axis=1)).astype(np.int64), nn - 1)
    i1 = np.minimum(np.floor(u.max(axis=1)).astype(np.int64), nn - 1)
    dims = i1 - i0 + 1
    counts = dims.prod(axis=1)
    nc = n[0] * n[1] * n[2]
    A, P = np.zeros(nc), np.zeros(nc)
    ends = np.cumsum(counts)
    t0 = 0
    while t0 < u.shape[0]:
        # as many whole triangles as fit a chunk (one at least)
        base = ends[t0 - 1] if t0 else 0
        t1 = max(int(np.searchsorted(ends, base + _SOLID_CHUNK, side='right')), t0 + 1)
        cn = counts[t0:t1]
        tri = np.repeat(np.arange(t0, t1), cn)
        local = np.arange(int(cn.sum())) - np.repeat(np.cumsum(cn) - cn, cn)
        d = dims[tri]
        cell = np.stack((local // (d[:, 1] * d[:, 2]), (local // d[:, 2]) % d[:, 1], local % d[:, 2]), axis=1) + i0[tri]
        a, p = solid_terms(u[tri], cell)
        q = (cell[:, 0] * n[1] + cell[:, 1]) * n[2] + cell[:, 2]
        A += np.bincount(q, weights=a, minlength=nc)
        P += np.bincount(q, weights=p, minlength=nc)
        t0 = t1
    A, P = A.reshape(n), P.reshape(n)
    beyond = np.cumsum(A[::-1], axis=0)[::-1] - A                          # sum over ix' > ix
    hh = np.asarray(h, dtype=np.float64).reshape(3)
    return (P + beyond) * (hh[0] * hh[1] * hh[2])


# ------------------------------------------------------------------------------------------------ VTK
def _vtk_order(a):
    """(nx, ny, nz[, k]) -> rows in VTK's cell order (x fastest)."""
    a = np.asarray(a, dtype=np.float64)
    return a.transpose(2, 1, 0).reshape(-1) if a.ndim == 3 else a.transpose(2, 1, 0, 3).reshape(-1, a.shape[3])


def write_vtk(path, lo, h, n, N, T, energy, heat_flux, title='nanokappa field', solid_fraction=None):
    """Legacy ASCII VTK, STRUCTURED_POINTS with CELL_DATA: scalars N, T, energy and the vector heat_flux (any viewer opens it;
    full float64 precision, NaN where a cell is empty).  solid_fraction (nx, ny, nz), where given, is one more scalar: it tells
    a cell outside the solid (0) from a cell no particle landed in; without it the file is what it always was."""
    n = tuple(int(k) for k in n)
    nc = n[0] * n[1] * n[2]
    T = np.full(n, np.nan) if T is None else T
    with open(path, 'w') as f:
        f.write('# vtk DataFile Version 3.0\n%s\nASCII\nDATASET STRUCTURED_POINTS\n' % title.replace('\n', ' ')[:255])
        f.write('DIMENSIONS %d %d %d\n' % (n[0] + 1, n[1] + 1, n[2] + 1))
        f.write('ORIGIN %.17g %.17g %.17g\n' % tuple(np.asarray(lo, dtype=float)))
        f.write('SPACING %.17g %.17g %.17g\n' % tuple(np.asarray(h, dtype=float)))
        f.write('CELL_DATA %d\n' % nc)
        scalars = [('N', N), ('T', T), ('energy', energy)]
        if solid_fraction is not None:
            scalars.append(('solid_fraction', np.asarray(solid_fraction, dtype=np.float64).reshape(n)))
        for name, a in scalars:
            f.write('SCALARS %s double 1\nLOOKUP_TABLE default\n' % name)
            f.write('\n'.join('%.17g' % x for x in _vtk_order(a)) + '\n')
        f.write('VECTORS heat_flux double\n')
        f.write('\n'.join('%.17g %.17g %.17g' % tuple(r) for r in _vtk_order(heat_flux)) + '\n')
    return path


def read_vtk(path):
    """What write_vtk wrote: dict lo, h, n, title, N, T, energy (nx, ny, nz), heat_flux (nx, ny, nz, 3), and solid_fraction
    (nx, ny, nz) where the file holds it."""
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
