"""Frequency-resolved conductivity: band maps, the per-connection band conductivity and its text output.

The reference computes it in Visualisation.flux_contribution (classes/Visualisation.py:592-651) from one snapshot of the
particles.  Here the engine tallies the band sums on the device (nk_set_bands: F[s][b] = sum v e, N[s][b] = particles), on
every heat-flux step or for the current state, and this module turns them into k(omega) per subvolume connection.
"""
import os

import numpy as np


def frequency_bands(omega, nbands):
    """Visualisation.py:609: edges = np.histogram_bin_edges(omega, nbands) over every mode, and the band of every mode by
    np.histogram's rule (bins half-open, the last one closed).  Returns (band_of_mode int32 [Q*J], edges [nbands + 1])."""
    om = np.asarray(omega, dtype=float).ravel()
    edges = np.histogram_bin_edges(om, int(nbands))
    band = np.searchsorted(edges, om, side='right') - 1
    band[om == edges[-1]] = int(nbands) - 1
    band[(om < edges[0]) | (om > edges[-1])] = -1
    return band.astype(np.int32), edges


def branch_bands(Q, J):
    """One band per branch: band of mode q*J+j is j.  Edges j - 1/2 (centres = branch indices)."""
    return np.tile(np.arange(J, dtype=np.int32), Q), np.arange(J + 1, dtype=float) - 0.5


def band_map(omega, nbands, kind='frequency'):
    """(band_of_mode, nbands, edges) for kind 'frequency' (nbands bins of omega [Q, J]), 'branch' (nbands is ignored: one per
    branch), or a caller-supplied array of the band of every global mode q*J+j (-1 = in no band; mean-free-path bands, ...),
    whose edges are then just the band indices +- 1/2."""
    omega = np.asarray(omega, dtype=float)
    if isinstance(kind, str):
        if kind == 'frequency':
            b, e = frequency_bands(omega, nbands)
            return b, int(nbands), e
        if kind == 'branch':
            Q, J = omega.shape
            b, e = branch_bands(Q, J)
            return b, J, e
        raise ValueError('unknown band kind %r (frequency, branch or an array)' % (kind,))
    b = np.ascontiguousarray(kind, dtype=np.int32).ravel()
    if b.shape[0] != omega.size:
        raise ValueError('band_of_mode has %d entries, the material %d modes' % (b.shape[0], omega.size))
    n = int(nbands) if nbands else int(b.max()) + 1
    if b.min() < -1 or b.max() >= n:
        raise ValueError('band_of_mode holds bands outside -1 .. %d' % (n - 1))
    return b, n, np.arange(n + 1, dtype=float) - 0.5


def connection_k(F, N, connections, con_vectors, T, active_modes, qv, eVpsa2_in_Wm2, a_in_m, n_sv=None):
    """k(omega) of every subvolume connection [C, B] from band sums F [S, B, 3], N [S, B] and the subvolume temperatures T [S]
    (the window means): Visualisation.py:598-637 summed by band.  There, every particle i of the connection's two subvolumes
    contributes -phi_i . dX / dT * active_modes / n (n = ALL particles of those subvolumes, :629-631) to the histogram bin of its
    frequency, with phi_i = normalise_to_density(hbar dn_i omega_i v_i) in W/m^2 (:604-605) and dX = subvol_con_vectors in m
    (:607); qv = number_of_qpoints * volume_unitcell (normalise_to_density).  n_sv [S]: particles per subvolume; without it n
    is the sum of N over the bands, the same for band maps that put every mode in a band (frequency, branch), fewer for a
    map with -1 entries.  The reference draws only the connections whose k is significant (:617-628); every one is returned."""
    F = np.asarray(F, dtype=float)
    N = np.asarray(N, dtype=float)
    con = np.asarray(connections, dtype=int).reshape(-1, 2)
    i, j = con[:, 0], con[:, 1]
    T = np.asarray(T, dtype=float)
    if n_sv is None:
        n = N[i].sum(axis=1) + N[j].sum(axis=1)
    else:
        n_sv = np.asarray(n_sv, dtype=float)
        n = n_sv[i] + n_sv[j]
    phi = (F[i] + F[j]) / qv * eVpsa2_in_Wm2                                   # [C, B, 3]
    dX = np.asarray(con_vectors, dtype=float).reshape(-1, 3) * a_in_m
    dT = T[j] - T[i]
    with np.errstate(divide='ignore', invalid='ignore'):
        k = -np.sum(phi * dX[:, None, :], axis=2) / dT[:, None]
        k = k * (active_modes / n)[:, None]
    return k


def write_k_contribution(path, edges, kind, connections, mean_k, std_k, steps=0):
    """k_contribution.txt: one line per band -- band, lower edge, upper edge, centre, then per connection mean k, std k and the
    cumulative sum of mean k over the bands up to this one (W/m K).  Edges in rad THz for frequency bands."""
    edges = np.asarray(edges, dtype=float)
    con = np.asarray(connections, dtype=int).reshape(-1, 2)
    mean_k = np.asarray(mean_k, dtype=float).reshape(con.shape[0], -1)
    std_k = np.asarray(std_k, dtype=float).reshape(con.shape[0], -1)
    B = edges.shape[0] - 1
    cols = [np.arange(B), edges[:-1], edges[1:], (edges[:-1] + edges[1:]) / 2]
    names = ['band', 'omega_lo', 'omega_hi', 'omega_centre']
    for c, (a, b) in enumerate(con):
        cols += [mean_k[c], std_k[c], np.cumsum(mean_k[c])]
        names += ['k_{:d}-{:d}'.format(a, b), 'sigma_k_{:d}-{:d}'.format(a, b), 'cum_k_{:d}-{:d}'.format(a, b)]
    data = np.column_stack(cols)
    header = ('frequency-resolved conductivity by subvolume connection, {:s} bands, mean over the convergence rows of the last '
              'n_mean window (up to step {:d})\n'.format(str(kind), int(steps)) + ' '.join(names))
    np.savetxt(path, data, fmt=['%6d'] + ['% .8e'] * (data.shape[1] - 1), header=header)
    return path


def read_k_contribution(path):
    """(edges, mean_k [C, B], std_k [C, B], cum_k [C, B]) of a k_contribution.txt."""
    d = np.atleast_2d(np.loadtxt(path))
    edges = np.append(d[:, 1], d[-1, 2])
    rest = d[:, 4:].T
    return edges, rest[0::3], rest[1::3], rest[2::3]


def k_contribution_path(folder):
    return os.path.join(folder, 'k_contribution.txt')
