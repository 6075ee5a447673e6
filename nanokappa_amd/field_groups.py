"""Grouped field maps: particle count N, deviational energy E = sum e_i and heat flux F = sum v_i e_i per (cell of the field's
grid, group of modes) -- where the heat goes AND which phonons carry it.  A group is a frequency bin, a branch, a
mean-free-path bin or a direction bin (or any table of the caller's).  The engine sums them (Engine.set_field_groups,
k_field_groups); this module is the host side, NumPy only and usable without a GPU: the option, the group builders, a float64
and a quantised restatement of the sums (what the tests hold the GPU against), the normalisation, and the file field_groups.npz.

Shapes: arrays per (cell, group) are (nx, ny, nz, G[, 3]); the grid convention is the field's (field.py)."""
import os

import numpy as np

from . import field as FD
from . import spectral

KINDS = ('frequency', 'branch', 'mfp', 'direction')
MAX_LINES = 1 << 24
_AXES = {'x': 0, 'y': 1, 'z': 2, '0': 0, '1': 1, '2': 2}


def field_groups_option(value):
    """--field_groups G kind [axis] -> (G, kind, axis); (0, None, None) when off (no value, or G = 0).  kind is one of
    frequency, branch, mfp, direction; axis (x, y, z or 0, 1, 2; direction only) is None where the slice axis is meant."""
    v = list(value or [])
    usage = ('--field_groups: expected G kind [axis] (G > 0 groups; kind one of %s; axis x, y or z, for direction), got %r'
             % (', '.join(KINDS), ' '.join(str(x) for x in v)))
    if not v:
        return 0, None, None
    try:
        G = int(v[0])
    except ValueError:
        raise ValueError(usage)
    if G == 0 and len(v) == 1:
        return 0, None, None
    if len(v) not in (2, 3) or G <= 0 or G > MAX_LINES:
        raise ValueError(usage)
    kind = str(v[1])
    if kind not in KINDS:
        raise ValueError(usage)
    axis = None
    if len(v) == 3:
        if kind != 'direction' or str(v[2]).lower() not in _AXES:
            raise ValueError(usage)
        axis = _AXES[str(v[2]).lower()]
    return G, kind, axis


def require_field(G, field_n):
    """--field_groups needs --field_grid: the groups live on the field's grid."""
    if G > 0 and field_n is None:
        raise ValueError('--field_groups requires --field_grid nx ny nz [every]: the groups are summed on the field\'s grid')


# ------------------------------------------------------------------------------------------------ group builders
def _moving(group_vel, inactive):
    v = np.asarray(group_vel, dtype=np.float64).reshape(-1, 3)
    speed = np.linalg.norm(v, axis=1)
    ok = speed > 0.0
    if inactive is not None:
        ok &= ~np.asarray(inactive, dtype=bool).ravel()
    return v, speed, ok


def frequency_groups(omega, G, inactive=None):
    """G bins of omega, spectral.band_map's (np.histogram's rule); inactive modes get -1.  -> (group_of_mode, G, edges)"""
    b, n, edges = spectral.band_map(omega, G, 'frequency')
    return _mask(b, inactive), n, edges


def branch_groups(omega, inactive=None):
    """One group per branch, spectral.band_map's; inactive modes get -1."""
    b, n, edges = spectral.band_map(omega, 0, 'branch')
    return _mask(b, inactive), n, edges


def _mask(b, inactive):
    b = np.array(b, dtype=np.int32).ravel()
    if inactive is not None:
        b[np.asarray(inactive, dtype=bool).ravel()] = -1
    return b


def mfp_groups(mfp, G, inactive=None):
    """G log-spaced bins of the mean free path [Q, J] (modes.mean_free_path) between the smallest and the largest positive one
    of the active modes; bins half-open, the last one closed.  Inactive modes and modes that do not move (mean free path 0,
    or not finite) get -1."""
    x = np.asarray(mfp, dtype=np.float64).ravel()
    ok = np.isfinite(x) & (x > 0.0)
    if inactive is not None:
        ok &= ~np.asarray(inactive, dtype=bool).ravel()
    G = int(G)
    g = np.full(x.shape[0], -1, dtype=np.int32)
    if not ok.any():
        return g, G, np.full(G + 1, np.nan)
    lo, hi = x[ok].min(), x[ok].max()
    if hi <= lo:
        hi = lo * (1.0 + 1e-9)
    edges = np.geomspace(lo, hi, G + 1)
    edges[0], edges[-1] = lo, hi
    b = np.searchsorted(edges, x[ok], side='right') - 1
    g[ok] = np.clip(b, 0, G - 1)
    return g, G, edges


def direction_groups(group_vel, G, axis=0, inactive=None):
    """G bins uniform in the cosine between v_g and the axis (0, 1, 2 or a vector): group = floor((cos + 1) G / 2), cos = 1 in
    the last one.  G = 2 splits by the sign of v . axis (a mode that flies exactly across the axis counts as forward).
    Inactive and zero-velocity modes get -1.  Edges are cosines, -1 .. 1."""
    v, speed, ok = _moving(group_vel, inactive)
    a = np.zeros(3)
    if np.ndim(axis) == 0:
        a[int(axis)] = 1.0
    else:
        a = np.asarray(axis, dtype=np.float64).reshape(3)
        a = a / np.linalg.norm(a)
    G = int(G)
    g = np.full(v.shape[0], -1, dtype=np.int32)
    cos = np.clip((v[ok] @ a) / speed[ok], -1.0, 1.0)
    g[ok] = np.minimum(np.floor((cos + 1.0) * (0.5 * G)).astype(np.int64), G - 1)
    return g, G, np.linspace(-1.0, 1.0, G + 1)


def build_groups(kind, G, phonon, T=None, axis=0):
    """(group_of_mode int32 [Q*J], G, edges) of a Phonon for kind frequency, branch (G follows the material), mfp (at
    temperature T, clipped into the material's range) or direction (against `axis`)."""
    inactive = getattr(phonon, 'inactive_modes_mask', None)
    if kind == 'frequency':
        return frequency_groups(phonon.omega, G, inactive)
    if kind == 'branch':
        return branch_groups(phonon.omega, inactive)
    if kind == 'mfp':
        from .modes import mean_free_path
        if T is None:
            raise ValueError("build_groups: 'mfp' needs a temperature")
        t = phonon.temperature_array
        return mfp_groups(mean_free_path(phonon, float(np.clip(T, t[0], t[-1]))), G, inactive)
    if kind == 'direction':
        return direction_groups(phonon.group_vel, G, 0 if axis is None else axis, inactive)
    raise ValueError('unknown group kind %r (%s)' % (kind, ', '.join(KINDS)))


# ------------------------------------------------------------------------------------------------ the sums on the host
def _lines(pos, group, lo, h, n, G):
    n = tuple(int(k) for k in n)
    c, out = FD.cell_index(pos, lo, h, n)
    g = np.asarray(group, dtype=np.int64).ravel()
    if g.shape[0] != c.shape[0] or (g.size and (g.min() < -1 or g.max() >= int(G))):
        raise ValueError('field_groups: one group in [-1, G) per particle is required')
    ok = g >= 0
    line = ((c[:, 0] * n[1] + c[:, 1]) * n[2] + c[:, 2]) * int(G) + g
    return n, line[ok], ok, int(out[ok].sum())


def groups_from_particles(pos, e, v, group, lo, h, n, G):
    """The sums in float64: dict N (nx, ny, nz, G), E, F (.., 3), clamped, ungrouped.  pos [P, 3], e [P], v [P, 3], group [P]
    (the group of every particle's mode; -1: added nowhere, counted in ungrouped)."""
    n, line, ok, clamped = _lines(pos, group, lo, h, n, G)
    nl = n[0] * n[1] * n[2] * int(G)
    e = np.asarray(e, dtype=np.float64).ravel()[ok]
    v = np.asarray(v, dtype=np.float64).reshape(-1, 3)[ok]
    sh = n + (int(G),)
    N = np.bincount(line, minlength=nl).astype(np.float64)
    E = np.bincount(line, weights=e, minlength=nl)
    F = np.stack([np.bincount(line, weights=v[:, a] * e, minlength=nl) for a in range(3)], axis=-1)
    return dict(N=N.reshape(sh), E=E.reshape(sh), F=F.reshape(sh + (3,)), clamped=clamped, ungrouped=int((~ok).sum()))


def quantised(pos, e, v, group, lo, h, n, G, k_E, k_F):
    """The same sums the way the GPU forms them (field.quantised per group): dict raw (nx, ny, nz, G, 8) int64 = {N, E 2^k_E,
    Fx 2^k_F, Fy 2^k_F, Fz 2^k_F, 0, 0, 0}, N, E, F (the reals they stand for), clamped, ungrouped.  With every particle in a
    group, raw summed over the groups equals field.quantised's raw bit for bit."""
    n, line, ok, clamped = _lines(pos, group, lo, h, n, G)
    nl = n[0] * n[1] * n[2] * int(G)
    e = np.asarray(e, dtype=np.float64).ravel()[ok]
    v = np.asarray(v, dtype=np.float64).reshape(-1, 3)[ok]
    raw = np.zeros((nl, 8), dtype=np.int64)
    np.add.at(raw[:, 0], line, 1)
    np.add.at(raw[:, 1], line, np.rint(np.ldexp(e, int(k_E))).astype(np.int64))
    for a in range(3):
        np.add.at(raw[:, 2 + a], line, np.rint(np.ldexp(v[:, a] * e, int(k_F))).astype(np.int64))
    sh = n + (int(G),)
    return dict(raw=raw.reshape(sh + (8,)), N=raw[:, 0].astype(np.float64).reshape(sh),
                E=np.ldexp(raw[:, 1].astype(np.float64), -int(k_E)).reshape(sh),
                F=np.ldexp(raw[:, 2:5].astype(np.float64), -int(k_F)).reshape(sh + (3,)), clamped=clamped, ungrouped=int((~ok).sum()))


def normalise(N, E, F, N_cell, samples, active_modes, QV, eVpsa2_in_Wm2, norm='mean', particle_density=None, cell_volume=None):
    """field.normalise per (cell, group).  The scale of a cell is computed from the cell's TOTAL count N_cell (nx, ny, nz) --
    the field's N -- and applied to every group of the cell, so the groups' energies and heat fluxes add up to the field's
    deviational energy and heat flux (for a table without ungrouped modes).  No reference energy is added: a group holds a
    share of the deviation.  For 'fixed', cell_volume is the whole cell's volume or, as in field.normalise, an array (nx, ny, nz)
    with the volume of solid in every cell (a cell of zero volume gives NaN).  Returns dict N (mean count per sample), energy
    (eV/angstrom^3), heat_flux (W/m^2); cells without particles are NaN."""
    N = np.asarray(N, dtype=np.float64)
    E = np.asarray(E, dtype=np.float64)
    F = np.asarray(F, dtype=np.float64)
    Nc = np.asarray(N_cell, dtype=np.float64)
    s = max(int(samples), 1)
    with np.errstate(divide='ignore', invalid='ignore'):
        if norm == 'fixed':
            if particle_density is None or cell_volume is None:
                raise ValueError("normalise: 'fixed' needs particle_density and cell_volume")
            FD.check_cell_volume(cell_volume, Nc.shape)
            scale = np.where(Nc > 0, active_modes / (particle_density * cell_volume * s), np.nan)
            scale = FD.mask_empty_volume(scale, cell_volume, Nc.shape)
        elif norm == 'mean':
            scale = np.where(Nc > 0, active_modes / Nc, np.nan)
        else:
            raise ValueError('normalise: norm must be mean or fixed')
        energy = E * scale[..., None] / QV
        flux = F * scale[..., None, None] / QV * eVpsa2_in_Wm2
    return dict(N=N / s, energy=energy, heat_flux=flux)


# ------------------------------------------------------------------------------------------------ field_groups.npz
_KEYS = ('lo', 'h', 'n', 'kind', 'edges', 'N', 'E', 'F', 'heat_flux', 'samples', 'step')


def write_field_groups(path, lo, h, n, kind, edges, N, E, F, heat_flux, samples, step, solid_fraction=None):
    """field_groups.npz: the grid (lo, h, n), the kind of the groups and their edges, the window's sums N, E (nx, ny, nz, G),
    F (.., 3), the normalised heat_flux (W/m^2), the number of samples in the sums and the step; where given, the solid
    fraction of every cell (nx, ny, nz) as one more array."""
    more = {} if solid_fraction is None else dict(solid_fraction=np.asarray(solid_fraction, dtype=np.float64))
    np.savez(path, lo=np.asarray(lo, dtype=np.float64), h=np.asarray(h, dtype=np.float64), n=np.asarray(n, dtype=np.int64),
             kind=np.asarray(str(kind)), edges=np.asarray(edges, dtype=np.float64), N=np.asarray(N, dtype=np.float64),
             E=np.asarray(E, dtype=np.float64), F=np.asarray(F, dtype=np.float64), heat_flux=np.asarray(heat_flux, dtype=np.float64),
             samples=np.int64(samples), step=np.int64(step), **more)
    return path


def read_field_groups(path):
    """What write_field_groups wrote, as a dict (kind a str, n a tuple, samples and step ints; solid_fraction where the file
    holds it)."""
    with np.load(path) as z:
        out = {k: z[k] for k in _KEYS}
        if 'solid_fraction' in z.files:
            out['solid_fraction'] = z['solid_fraction']
    out['kind'] = str(out['kind'])
    out['n'] = tuple(int(k) for k in out['n'])
    out['samples'], out['step'] = int(out['samples']), int(out['step'])
    return out


def field_groups_path(folder):
    return os.path.join(folder, 'field_groups.npz')
