"""Mode-resolved tally: E[s][m] = sum e_i and N[s][m] over the particles of subvolume s in mode m = q*J + j -- the solution of
the Boltzmann equation itself, at full resolution.  The engine sums the table (Engine.set_modes, k_modes); this module is the
host side, NumPy only and usable without a GPU: a float64 restatement of the sums and of the integer sums the GPU forms (what
the tests hold the GPU against), and what one reads off the table -- the heat flux of every mode (v_m E: the group velocity is
a property of the mode), the mean deviation of its occupation, its contribution to the conductivity of every subvolume
connection, and the conductivity accumulated over the mean free path or the frequency.

Shapes: tables are [S, M] (or [S, Q, J], which is the same memory); k per connection and mode is [C, M]."""
import os

import numpy as np

from . import spectral


def mode_tally_option(value, n_dt_to_conv=10):
    """--mode_tally [every] -> every; 0 = off (the option is absent, or given as 0).  Given without a value the cadence is the
    field's default (field.FIELD_EVERY_DEFAULT); otherwise a positive multiple of n_dt_to_conv (the heat-flux cadence)."""
    from .field import FIELD_EVERY_DEFAULT
    if value is None:
        return 0
    v = list(value) if isinstance(value, (list, tuple)) else [value]
    usage = '--mode_tally: expected [every], a positive multiple of n_dt_to_conv (%d), got %r' % (int(n_dt_to_conv),
                                                                                                 ' '.join(str(x) for x in v))
    if len(v) == 0:
        every = FIELD_EVERY_DEFAULT
    elif len(v) == 1:
        try:
            every = int(v[0])
        except ValueError:
            raise ValueError(usage)
    else:
        raise ValueError(usage)
    if every == 0:
        return 0
    if every < 0 or int(n_dt_to_conv) <= 0 or every % int(n_dt_to_conv) != 0:
        raise ValueError(usage)
    return every


def _bins(sv, mode, S, M):
    sv = np.asarray(sv, dtype=np.int64).ravel()
    mode = np.asarray(mode, dtype=np.int64)
    if mode.ndim == 2:                                   # (q, j) pairs need J: refuse rather than guess
        raise ValueError('mode must be the global index q*J + j')
    mode = mode.ravel()
    if sv.shape != mode.shape:
        raise ValueError('sv and mode must have one entry per particle')
    if sv.size and (sv.min() < 0 or sv.max() >= S or mode.min() < 0 or mode.max() >= M):
        raise ValueError('a subvolume or mode index is outside the table')
    return sv * int(M) + mode


def table_from_particles(sv, mode, e, S, M):
    """The sums in float64: dict N, E [S, M].  sv [P] subvolume, mode [P] global mode q*J + j, e [P] of every particle."""
    S, M = int(S), int(M)
    b = _bins(sv, mode, S, M)
    e = np.asarray(e, dtype=np.float64).ravel()
    N = np.bincount(b, minlength=S * M).astype(np.float64)
    E = np.bincount(b, weights=e, minlength=S * M)
    return dict(N=N.reshape(S, M), E=E.reshape(S, M))


def quantised(sv, mode, e, S, M, k_E):
    """The same sums the way the GPU forms them: every term scaled by 2^k_E, rounded to nearest (rint) and added as int64.
    dict N_raw, E_raw [S, M] int64 and N, E, the reals they stand for.  Equal to the engine's integers bit for bit whenever
    the host's terms equal the device's; per bin E differs from the float64 sum by at most n_bin 2^-(k_E + 1)."""
    S, M = int(S), int(M)
    b = _bins(sv, mode, S, M)
    e = np.asarray(e, dtype=np.float64).ravel()
    Nr = np.zeros(S * M, dtype=np.int64)
    Er = np.zeros(S * M, dtype=np.int64)
    np.add.at(Nr, b, 1)
    np.add.at(Er, b, np.rint(np.ldexp(e, int(k_E))).astype(np.int64))
    return dict(N_raw=Nr.reshape(S, M), E_raw=Er.reshape(S, M), N=Nr.astype(np.float64).reshape(S, M),
                E=np.ldexp(Er.astype(np.float64), -int(k_E)).reshape(S, M))


def _flat(a, ndim_tail=0):
    """[S, Q, J, ...] or [S, M, ...] -> [S, M, ...]"""
    a = np.asarray(a, dtype=np.float64)
    return a.reshape((a.shape[0], -1) + a.shape[a.ndim - ndim_tail:]) if ndim_tail else a.reshape(a.shape[0], -1)


def mode_flux(E, group_vel):
    """Heat flux sum of every (subvolume, mode), [S, M, 3] = v_m E[s][m]: exact, since every particle of a mode has its
    velocity.  group_vel [Q, J, 3] or [M, 3]."""
    E = _flat(E)
    v = np.asarray(group_vel, dtype=np.float64).reshape(-1, 3)
    if v.shape[0] != E.shape[1]:
        raise ValueError('group_vel has %d modes, the table %d' % (v.shape[0], E.shape[1]))
    return E[:, :, None] * v[None, :, :]


def occupation_deviation(E, N, omega, hbar):
    """Mean deviation of the occupation of every (subvolume, mode) from the reference occupation, E / (hbar omega_m N);
    NaN where a bin holds no particle (or omega = 0)."""
    E, N = _flat(E), _flat(N)
    om = np.asarray(omega, dtype=np.float64).ravel()
    with np.errstate(divide='ignore', invalid='ignore'):
        return np.where(N > 0, E / (hbar * om[None, :] * N), np.nan)


def mode_k(E, N, group_vel, connections, con_vectors, T, active_modes, qv, eVpsa2_in_Wm2, a_in_m, n_sv=None):
    """Conductivity contribution of every mode to every subvolume connection, [C, M]: spectral.connection_k with one band per
    mode.  connection_k is linear in F for a given n, and n is ALL particles of the connection's two subvolumes here (n_sv [S],
    by default the sum of N over the modes), so for ANY band_of_mode the values summed by band equal connection_k of the band
    sums called with the same n_sv."""
    E, N = _flat(E), _flat(N)
    if n_sv is None:
        n_sv = N.sum(axis=1)
    return spectral.connection_k(mode_flux(E, group_vel), N, connections, con_vectors, T, active_modes, qv, eVpsa2_in_Wm2, a_in_m,
                                 n_sv=n_sv)


def band_sums(a, band_of_mode, nbands):
    """Sum a [..., M] over the modes of every band -> [..., nbands]; modes in band -1 are left out."""
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(band_of_mode, dtype=np.int64).ravel()
    ok = b >= 0
    out = np.zeros((int(nbands),) + a.shape[:-1])
    np.add.at(out, b[ok], np.moveaxis(a[..., ok], -1, 0))
    return np.moveaxis(out, 0, -1)


def mean_free_path(phonon, T):
    """|v_m| tau_m(T) of every mode [Q, J] (angstrom): group speed times Phonon.lifetime_function at temperature T."""
    Q, J = phonon.omega.shape
    q, j = np.meshgrid(np.arange(Q), np.arange(J), indexing='ij')
    Tqj = np.stack([np.full(Q * J, float(T)), q.ravel(), j.ravel()], axis=1)
    tau = np.asarray(phonon.lifetime_function(Tqj), dtype=np.float64).reshape(Q, J)
    return np.linalg.norm(np.asarray(phonon.group_vel, dtype=np.float64), axis=2) * tau


def accumulation(k_mode, x, grid):
    """Cumulative conductivity over a per-mode quantity x (mean free path, frequency): out[..., i] = sum of k_mode[..., m] over
    the modes with x[m] <= grid[i].  k_mode [M] or [C, M]; grid must not decrease.  Modes whose x is NaN are in no point."""
    k = np.asarray(k_mode, dtype=np.float64)
    x = np.asarray(x, dtype=np.float64).ravel()
    grid = np.asarray(grid, dtype=np.float64).ravel()
    if k.shape[-1] != x.shape[0]:
        raise ValueError('k_mode has %d modes, x %d' % (k.shape[-1], x.shape[0]))
    if np.any(np.isnan(grid)) or np.any(np.diff(grid) < 0):
        raise ValueError('accumulation: the grid must not decrease')
    ok = ~np.isnan(x)
    order = np.argsort(x[ok], kind='stable')
    xs = x[ok][order]
    cum = np.concatenate([np.zeros(k.shape[:-1] + (1,)), np.cumsum(k[..., ok][..., order], axis=-1)], axis=-1)
    return cum[..., np.searchsorted(xs, grid, side='right')]


def accumulation_grid(x, points=200, log=True):
    """A grid for accumulation(): `points` values from the smallest positive to the largest finite x (logarithmic or linear
    spacing); the last one IS the largest x, so the last accumulation point is the total."""
    x = np.asarray(x, dtype=np.float64).ravel()
    x = x[np.isfinite(x)]
    hi = float(x.max()) if x.size else 1.0
    pos = x[x > 0]
    lo = float(pos.min()) if pos.size else hi
    if not (hi > lo):
        return np.array([hi])
    g = np.geomspace(lo, hi, int(points)) if log and lo > 0 else np.linspace(lo, hi, int(points))
    g[-1] = hi
    return g


def write_k_accumulation(path, grid, cum_k, connections, by='mfp', steps=0):
    """k_accumulation.txt: one line per grid point -- the mean free path (angstrom; by='mfp') or the frequency (rad THz;
    by='frequency'), then the cumulative k of every connection (W/m K)."""
    con = np.asarray(connections, dtype=int).reshape(-1, 2)
    cum_k = np.asarray(cum_k, dtype=np.float64).reshape(con.shape[0], -1)
    grid = np.asarray(grid, dtype=np.float64).ravel()
    names = ['mean_free_path' if by == 'mfp' else 'omega'] + ['cum_k_{:d}-{:d}'.format(a, b) for a, b in con]
    header = ('conductivity accumulated over the {:s} of the modes, by subvolume connection, from the mode-resolved tally of the '
              'last n_mean window (up to step {:d})\n'.format('mean free path' if by == 'mfp' else 'frequency', int(steps)) +
              ' '.join(names))
    np.savetxt(path, np.column_stack([grid] + [c for c in cum_k]), fmt='% .17e', header=header)
    return path


def read_k_accumulation(path):
    """(grid [G], cum_k [C, G]) of a k_accumulation.txt."""
    d = np.atleast_2d(np.loadtxt(path))
    return d[:, 0], d[:, 1:].T


def write_mode_tally(path, N, E, samples, step, omega, group_vel):
    """mode_tally.npz: the window's sums N, E [S, Q, J], the number of samples in them, the step, omega [Q, J], group_vel."""
    om = np.asarray(omega, dtype=np.float64)
    np.savez_compressed(path, N=np.asarray(N, dtype=np.float64).reshape((-1,) + om.shape),
                        E=np.asarray(E, dtype=np.float64).reshape((-1,) + om.shape), samples=np.int64(samples), step=np.int64(step),
                        omega=om, group_vel=np.asarray(group_vel, dtype=np.float64))
    return path


def read_mode_tally(path):
    with np.load(path) as z:
        return {k: z[k] for k in z.files}


def k_accumulation_path(folder, by='mfp'):
    return os.path.join(folder, 'k_accumulation.txt' if by == 'mfp' else 'k_accumulation_frequency.txt')


def mode_tally_path(folder):
    return os.path.join(folder, 'mode_tally.npz')
