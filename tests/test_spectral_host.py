"""Frequency-resolved conductivity, host side (no GPU): band maps, the per-connection k(omega) against a restatement of the
reference's Visualisation.flux_contribution (Visualisation.py:598-637), the option's default and k_contribution.txt."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
sys.path.insert(0, ROOT)

from nanokappa_amd import spectral as SP
from nanokappa_amd.constants import Constants

K = Constants()


def test_frequency_bands_follow_np_histogram():
    rng = np.random.default_rng(1)
    omega = rng.random((50, 6)) * 80.0
    omega[3, 2] = omega.max() + 1.0          # a mode exactly on the top edge
    omega[0, 0] = 0.0
    for nb in (1, 7, 100):
        band, edges = SP.frequency_bands(omega, nb)
        assert np.array_equal(edges, np.histogram_bin_edges(omega, nb))
        assert band.min() >= 0 and band.max() == nb - 1
        assert np.array_equal(np.bincount(band, minlength=nb), np.histogram(omega, edges)[0])
        # a mode on an interior edge goes to the band above it, like np.histogram
        inner = edges[nb // 2]
        b, _ = SP.frequency_bands(np.append(omega.ravel(), inner), nb)
        assert np.array_equal(np.bincount(b, minlength=nb), np.histogram(np.append(omega.ravel(), inner), edges)[0])
    assert SP.frequency_bands(omega, 7)[0][3 * 6 + 2] == 6


def test_band_map_kinds():
    omega = np.arange(24, dtype=float).reshape(4, 6)
    b, n, e = SP.band_map(omega, 3, 'branch')
    assert n == 6 and np.array_equal(b, np.tile(np.arange(6), 4)) and e.shape == (7,)
    custom = np.arange(24) % 5 - 1
    b, n, e = SP.band_map(omega, 4, custom)
    assert n == 4 and np.array_equal(b, custom)
    with pytest.raises(ValueError):
        SP.band_map(omega, 3, custom)
    with pytest.raises(ValueError):
        SP.band_map(omega, 3, 'wavelength')


def reference_k(subvol_id, omega_p, v_p, dn, con, con_vectors, mean_T, active_modes, qv, bins):
    """Visualisation.py:598-637 restated: per connection the histogram of omega with weights k_i."""
    hbar = K.hbar
    phi = (hbar * dn.reshape(-1, 1) * omega_p.reshape(-1, 1) * v_p) / qv
    phi *= K.eVpsa2_in_Wm2
    dX = con_vectors * K.a_in_m
    dT = mean_T[con[:, 1]] - mean_T[con[:, 0]]
    out = []
    for c, cc in enumerate(con):
        i = np.logical_or(subvol_id == cc[0], subvol_id == cc[1]).nonzero()[0]
        k = -np.sum(phi[i, :] * dX[c, :], axis=1) / dT[c]
        k *= active_modes / k.shape[0]
        y, _ = np.histogram(omega_p[i], bins=bins, weights=k)
        out.append(y)
    return np.array(out)


@pytest.mark.parametrize('layout', ['slice', 'grid'])
def test_connection_k_matches_reference_formula(layout):
    rng = np.random.default_rng(3)
    Q, J, n = 40, 6, 20000
    omega = rng.random((Q, J)) * 70.0 + 1.0
    vg = rng.normal(size=(Q * J, 3)) * 30.0
    if layout == 'slice':
        S = 5
        centers = np.stack([np.linspace(10, 90, S), np.full(S, 50.0), np.full(S, 50.0)], axis=1)
        con = np.stack([np.arange(S - 1), np.arange(1, S)], axis=1)
    else:
        g = np.array([[x, y, 50.0] for x in (25.0, 75.0) for y in (25.0, 75.0)])
        centers, S = g, 4
        con = np.array([[0, 1], [0, 2], [1, 3], [2, 3]])
    con_vectors = centers[con[:, 1]] - centers[con[:, 0]]
    sv = rng.integers(0, S, n)
    mode = rng.integers(0, Q * J, n)
    dn = rng.normal(size=n) * 1e-2 + np.where(sv % 2 == 0, 2e-3, -1e-3)
    om_p = omega.ravel()[mode]
    v_p = vg[mode]
    mean_T = 300.0 + np.arange(S) * 0.7
    qv = 123.4
    B = 100
    band, edges = SP.frequency_bands(omega, B)
    e = K.hbar * om_p * dn
    b = band[mode]
    F = np.zeros((S, B, 3))
    for d in range(3):
        F[:, :, d] = np.bincount(sv * B + b, weights=v_p[:, d] * e, minlength=S * B).reshape(S, B)
    N = np.bincount(sv * B + b, minlength=S * B).reshape(S, B).astype(float)
    k = SP.connection_k(F, N, con, con_vectors, mean_T, Q * J, qv, K.eVpsa2_in_Wm2, K.a_in_m)
    ref = reference_k(sv, om_p, v_p, dn, con, con_vectors, mean_T, Q * J, qv, edges)
    assert k.shape == ref.shape == (con.shape[0], B)
    assert np.max(np.abs(k - ref)) <= 1e-12 * np.max(np.abs(ref))


def test_parser_default_is_off():
    from nanokappa_amd.argument_parser import initialise_parser
    a = initialise_parser().parse_args(['--poscar_file', 'P', '--hdf_file', 'h'])
    assert int(a.spectral_bands[0]) == 0
    a = initialise_parser().parse_args(['--poscar_file', 'P', '--hdf_file', 'h', '--spectral_bands', '20', 'branch'])
    assert a.spectral_bands == ['20', 'branch']


def test_k_contribution_layout(tmp_path):
    edges = np.linspace(0.0, 80.0, 11)
    con = np.array([[0, 1], [1, 2]])
    mk = np.arange(20, dtype=float).reshape(2, 10) - 5.0
    sk = np.abs(mk) * 0.1
    path = SP.write_k_contribution(str(tmp_path / 'k_contribution.txt'), edges, 'frequency', con, mk, sk, steps=200)
    lines = open(path).read().splitlines()
    assert lines[0].startswith('# frequency-resolved conductivity')
    assert lines[1].split()[1:] == ['band', 'omega_lo', 'omega_hi', 'omega_centre', 'k_0-1', 'sigma_k_0-1', 'cum_k_0-1',
                                    'k_1-2', 'sigma_k_1-2', 'cum_k_1-2']
    d = np.loadtxt(path)
    assert d.shape == (10, 4 + 3 * 2)
    assert np.array_equal(d[:, 0], np.arange(10))
    e, m, s, c = SP.read_k_contribution(path)
    assert np.allclose(e, edges) and np.allclose(m, mk) and np.allclose(s, sk) and np.allclose(c, np.cumsum(mk, axis=1))
    assert np.allclose(d[:, 3], (edges[:-1] + edges[1:]) / 2)


def test_new_symbols_are_declared():
    from nanokappa_amd import engine
    for n in ('nk_set_bands', 'nk_get_band_rows', 'nk_tally_bands_state'):
        assert n in engine.EXPORTS
        assert n + '(' in open(os.path.join(ROOT, 'include', 'nanokappa_hip.h')).read()


def test_host_formula_against_reference_golden():
    """tests/golden/k_contribution.npz pins the reference's own Visualisation.flux_contribution on the post-step state of
    step.npz (make_k_contribution.py).  The band sums of that state, fed through connection_k, must give the same k(omega):
    same band edges, temperatures, particle counts and normalisation."""
    from util import golden, sub, golden_phonon
    kc = golden('k_contribution')
    gs = sub(golden('step'), 'lin')
    ph = golden_phonon()
    band, edges = SP.frequency_bands(ph.omega, 100)
    assert np.array_equal(edges, kc['bins'])
    m = gs['mid_modes'][:, 0] * ph.number_of_branches + gs['mid_modes'][:, 1]
    om = ph.omega.ravel()[m]
    e = ph.hbar * om * (gs['post_occupation'] - ph.calculate_occupation(gs['post_temperatures'], om))
    v = ph.group_vel.reshape(-1, 3)[m]
    sv = gs['post_subvol_id'].astype(int)
    S, B = gs['post_subvol_temperature'].shape[0], 100
    F = np.zeros((S, B, 3))
    for d in range(3):
        F[:, :, d] = np.bincount(sv * B + band[m], weights=v[:, d] * e, minlength=S * B).reshape(S, B)
    N = np.bincount(sv * B + band[m], minlength=S * B).reshape(S, B).astype(float)
    k = SP.connection_k(F, N, kc['subvol_connections'], kc['subvol_con_vectors'], kc['mean_T'], int(kc['number_of_active_modes']),
                        ph.number_of_qpoints * ph.volume_unitcell, K.eVpsa2_in_Wm2, K.a_in_m)
    y = kc['y']
    assert k.shape == y.shape
    assert np.max(np.abs(k - y)) <= 1e-12 * np.max(np.abs(y))
    n_sv = np.bincount(sv, minlength=S)
    k2 = SP.connection_k(F, N, kc['subvol_connections'], kc['subvol_con_vectors'], kc['mean_T'], int(kc['number_of_active_modes']),
                         ph.number_of_qpoints * ph.volume_unitcell, K.eVpsa2_in_Wm2, K.a_in_m, n_sv=n_sv)
    assert np.max(np.abs(k2 - y)) <= 1e-12 * np.max(np.abs(y))


def test_spectral_bands_option():
    from nanokappa_amd.population import spectral_bands_option as opt
    assert opt(None) == (0, 'frequency') and opt(['0', 'frequency']) == (0, 'frequency')
    assert opt(['100']) == (100, 'frequency') and opt(['20', 'branch']) == (20, 'branch') and opt(['branch']) == (1, 'branch')
    for bad in (['frequency'], ['x'], ['-1'], ['10', 'wavelength'], ['10', 'branch', '3']):
        with pytest.raises(ValueError) as e:
            opt(bad)
        assert '--spectral_bands' in str(e.value)
