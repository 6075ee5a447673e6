"""Band-resolved heat flux on the GPU (nk_set_bands / k_spectral): per band against the oracle's particles, the sum over the
bands against flux_raw, bands on leaving every other output alone, the state snapshot, the Population outputs and the
communicator path."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from util import case_tables, random_population, make_oracle_sim, make_engine, allclose, same_event_rule, TOL_T, TOL_X, TOL_OCC

pytestmark = pytest.mark.gpu

# F against the oracle's sums: both add the same ~1e4 terms of either sign in different orders.  Relative to the largest |F| of
# the row; 10x the largest deviation measured on the MI355X (4.6e-14 over the six cases of test_bands_against_oracle).
TOL_BAND_F = 5e-13
# k(omega) of state mode against the reference's own flux_contribution, relative to the largest |k|: the engine's per-particle
# temperatures and occupations against the reference's, summed by band; 10x the deviation measured on the MI355X (1.5e-14)
TOL_K_GOLDEN = 2e-13
# With tiles of bands and modes in no band, relative to the largest |value| of the row: the sum over the bands against flux_raw less
# the particles in no band, and flux_raw against the oracle's particles; 10x the deviation measured on the MI355X (1.5e-14, 1.6e-14)
TOL_BAND_SUM = 1.5e-13
# ... the state mode against the host formula (measured 1.6e-16)
TOL_BAND_STATE = 1.5e-15


def band_table(ct, nbands, kind):
    from nanokappa_amd import spectral as SP
    b, n, _ = SP.band_map(ct['ph'].omega, nbands, kind)
    return b, n


def oracle_bands(sim, ct, band, B):
    P = sim.P
    n = P.N
    S = ct['centers'].shape[0]
    sv, mode, e = P.sv[:n].astype(int), P.mode[:n].astype(int), P.energy[:n]
    v = np.asarray(ct['tables']['group_vel']).reshape(-1, 3)[mode]
    F, N = np.zeros((S, B, 3)), np.zeros((S, B))
    b = band[mode]
    keep = b >= 0
    for d in range(3):
        np.add.at(F[:, :, d], (sv[keep], b[keep]), v[keep, d] * e[keep])
    np.add.at(N, (sv[keep], b[keep]), 1.0)
    return F, N


def rel_rows(a, b):
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))


@pytest.mark.parametrize('case,nbands,kind,nobox', [('ttp', 1, 'frequency', False), ('ttp', 7, 'frequency', False),
                                                    ('ttp', 100, 'frequency', True), ('ttrrp', 100, 'frequency', False),
                                                    ('ttrrp', 7, 'frequency', True), ('ttrrp', 0, 'branch', False)])
def test_bands_against_oracle(case, nbands, kind, nobox, monkeypatch):
    if nobox:
        monkeypatch.setenv('NK_NO_BOX', '1')
    ct = case_tables(case)
    pos, mode, occ, counter = random_population(ct, 20000, seed=5)
    sim = make_oracle_sim(ct, pos, mode, occ, counter, seed=3)
    eng = make_engine(ct, pos, mode, occ, counter, seed=3)
    same_event_rule(eng, sim)
    band, B = band_table(ct, nbands, kind)
    eng.set_bands(band, B)
    t = eng.step(30)
    assert list(t['band_steps']) == [9, 19, 29]
    worst = 0.0
    for s in range(30):
        sim.run_timestep()
        if (s + 1) % 10:
            continue
        r = list(t['band_steps']).index(s)
        F0, N0 = oracle_bands(sim, ct, band, B)
        assert np.array_equal(t['band_N'][r], N0), 'band counts differ at step %d' % s
        d = rel_rows(t['band_F'][r], F0)
        worst = max(worst, d)
        assert d <= TOL_BAND_F, 'band flux differs at step %d: %.3e' % (s, d)
        fs = t['band_F'][r].sum(axis=1)
        assert rel_rows(fs, t['flux_raw'][s]) <= 1e-12
        assert np.array_equal(t['band_N'][r].sum(axis=1), t['N_sv'][s])
    print('band flux against the oracle, largest relative deviation %.3e' % worst)


def _sum_check(pop, nsteps):
    t = pop.engine.step(nsteps)
    assert t['band_steps'].shape[0] >= 2
    for r, st in enumerate(t['band_steps']):
        s = int(st) - int(pop.engine.get_step()) + nsteps
        assert rel_rows(t['band_F'][r].sum(axis=1), t['flux_raw'][s]) <= 1e-12, 'step %d' % st
        assert np.array_equal(t['band_N'][r].sum(axis=1), t['N_sv'][s])


def test_band_sum_equals_flux_config2():
    """BASELINE config 2 at full size (1e7 particles, box store, alternating walk): sum over 100 bands = flux_raw."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
    from test_gpu_fullsize import build
    pop, geo, ph = build('c2', 10000000)
    pop.set_bands('frequency', 100)
    _sum_check(pop, 30)


def test_band_sum_equals_flux_wire():
    """The 5000-face STL wire (split sweep, k_events, rough walls with migration): sum over the bands = flux_raw."""
    import bench
    from nanokappa_amd import synthetic
    from nanokappa_amd.phonon import Phonon
    from nanokappa_amd.population import Population
    args, geo = bench.wire_geometry(200000)
    ph = Phonon(args, 0, material=synthetic.make_material(9, 'Si', temperatures=np.arange(200.0, 401.0, 10.0)))
    pop = bench.quiet(Population, args, geo, ph)
    assert pop.engine.L is not None
    pop.set_bands('frequency', 20)
    _sum_check(pop, 20)


@pytest.mark.parametrize('case,gen', [('ttp', 0), ('ttrrp', 0), ('ttp', 2)])
def test_bands_leave_everything_else(case, gen):
    ct = case_tables(case)
    pos, mode, occ, counter = random_population(ct, 20000, seed=8)
    runs = []
    for on in (False, True):
        eng = make_engine(ct, pos, mode, occ, counter, seed=4, gen=gen)
        if on:
            band, B = band_table(ct, 100, 'frequency')
            eng.set_bands(band, B)
        t = eng.step(25)
        runs.append((t, eng.download()))
    (t0, p0), (t1, p1) = runs
    for k in ('N_sv', 'N_leaving', 'N_emitted'):
        assert np.array_equal(t0[k], t1[k]), k
    assert allclose(t0['T_sv'], t1['T_sv'], rtol=0, atol=TOL_T)
    i0, i1 = np.argsort(p0['pid']), np.argsort(p1['pid'])
    assert np.array_equal(p0['pid'][i0], p1['pid'][i1])
    assert np.array_equal(p0['mode'][i0], p1['mode'][i1])
    assert allclose(p0['positions'][i0], p1['positions'][i1], rtol=0, atol=TOL_X)
    assert allclose(p0['occupation'][i0], p1['occupation'][i1], rtol=TOL_OCC, atol=0)
    assert 'band_F' not in t0 and t1['band_F'].shape == (2, ct['centers'].shape[0], 100, 3)


def test_state_mode_against_host():
    """nk_tally_bands_state: occupations after the relaxation, n0 at each particle's interpolated temperature."""
    ct = case_tables('ttp')
    pos, mode, occ, counter = random_population(ct, 20000, seed=12)
    eng = make_engine(ct, pos, mode, occ, counter, seed=2)
    band, B = band_table(ct, 100, 'frequency')
    eng.set_bands(band, B)
    eng.step(7)
    F, N = eng.tally_bands_state()
    p = eng.download()
    x, m, n = p['positions'], p['mode'].astype(int), p['occupation']
    S = ct['centers'].shape[0]
    sv = eng.classify(x)
    T = eng.eval('interp_T', x)
    om = ct['ph'].omega.ravel()[m]
    n0 = np.where(T > 0, eng.eval('occupation', T, m), 0.0)
    e = ct['ph'].hbar * om * (n - n0)
    v = np.asarray(ct['tables']['group_vel']).reshape(-1, 3)[m]
    F0, N0 = np.zeros((S, B, 3)), np.zeros((S, B))
    for d in range(3):
        np.add.at(F0[:, :, d], (sv, band[m]), v[:, d] * e)
    np.add.at(N0, (sv, band[m]), 1.0)
    assert np.array_equal(N, N0)
    assert rel_rows(F, F0) <= 1e-11


def test_population_end_to_end(tmp_path):
    """A parameter-file run with --spectral_bands 100 writes k_contribution.txt; on every row the band flux adds up to the
    row's subvol_heat_flux."""
    import bench
    from nanokappa_amd import nanokappa, spectral as SP
    argv, species, _ = bench.config_argv('c2', 100000, 200.0)
    argv = argv + ['--seed', '7', '--spectral_bands', '100', 'frequency', '--iterations', '120', '--results_folder',
                   str(tmp_path / 'run'), '--n_mean', '5']
    pf = tmp_path / 'params.txt'
    pf.write_text(' '.join(argv))
    cwd = os.getcwd()
    os.chdir(str(tmp_path))
    try:
        pop = nanokappa.main(['-ff', str(pf)])
    finally:
        sys.stdout = sys.__stdout__
        os.chdir(cwd)
    path = SP.k_contribution_path(pop.results_folder_name)
    assert os.path.exists(path)
    edges, mk, sk, ck = SP.read_k_contribution(path)
    C = pop._geo.subvol_connections.shape[0]
    assert edges.shape == (101,) and mk.shape == (C, 100) and np.allclose(ck, np.cumsum(mk, axis=1), rtol=1e-6, atol=0)
    rows = [r for r in pop.conv_rows if 'band_F' in r]
    assert len(rows) == 12
    ph = pop._ph
    for r in rows:
        phi = pop._normalise_flux(ph, r['band_F'].sum(axis=1), r['sv_Np'])
        assert rel_rows(phi, r['phi']) <= 1e-12
    fc = pop.flux_contribution()
    assert fc['k'].shape == (C, 100) and np.all(np.isfinite(fc['k']))


def test_rows_through_single_rank_communicator(monkeypatch):
    from nanokappa_amd.engine import comm_unique_id
    ct = case_tables('ttp')
    pos, mode, occ, counter = random_population(ct, 20000, seed=9)
    band, B = band_table(ct, 20, 'frequency')
    ref = make_engine(ct, pos, mode, occ, counter, seed=1)
    ref.set_bands(band, B)
    t0 = ref.step(20)
    monkeypatch.setenv('NK_FORCE_COMM', '1')
    eng = make_engine(ct, pos, mode, occ, counter, seed=1)
    eng.comm_init(comm_unique_id(), 0, 1)
    eng.set_bands(band, B)
    t1 = eng.step(20)
    assert np.array_equal(t0['band_steps'], t1['band_steps'])
    assert np.array_equal(t0['band_N'], t1['band_N'])
    assert rel_rows(t1['band_F'], t0['band_F']) <= 1e-12
    F0, N0 = ref.tally_bands_state()
    F1, N1 = eng.tally_bands_state()
    assert np.array_equal(N0, N1) and rel_rows(F1, F0) <= 1e-12



def test_state_mode_against_reference_golden():
    """The reference's own Visualisation.flux_contribution on the post-step state of step.npz (tests/golden/
    k_contribution.npz, make_k_contribution.py) against Population.flux_contribution() over the engine's state mode: that
    state uploaded with its subvolume temperatures, k(omega) per connection with dT of the same temperatures."""
    import types
    from util import golden, sub, golden_phonon
    from nanokappa_amd.engine import Engine
    from nanokappa_amd.population import Population
    from nanokappa_amd.constants import Constants
    kc = golden('k_contribution')
    gm = sub(golden('mesh'), 'box200ttp')
    gs = sub(golden('step'), 'lin')
    ph = golden_phonon()
    J = ph.number_of_branches
    M = ph.number_of_qpoints * J
    eng = Engine(0, 1)
    eng.set_material(ph.tables())
    eng.set_mesh(gm)
    eng.set_subvolumes(gm['subvol_center'], gm['subvol_volume'], 0, int(gm['slice_axis']), 1, gs['post_subvol_temperature'])
    eng.set_reservoirs(gm['res_facets'], gs['res_facet_temperature'], np.zeros((2, M)), np.zeros((2, M)))
    eng.set_params(dt=1.0, particle_density=float(gs['particle_density']), flux_every=1, contains_every=0, track_ids=True)
    eng.upload(gs['mid_positions'], gs['mid_modes'][:, 0] * J + gs['mid_modes'][:, 1], gs['post_occupation'],
               gs['mid_n_timesteps'], gs['mid_collision_facets'])
    pop = Population.__new__(Population)
    Constants.__init__(pop)
    pop.engine, pop._ph, pop.nranks, pop.n_bands = eng, ph, 1, 0
    pop._geo = types.SimpleNamespace(subvol_connections=kc['subvol_connections'], subvol_con_vectors=kc['subvol_con_vectors'])
    pop.set_bands('frequency', 100, ph)
    fc = pop.flux_contribution(T=kc['mean_T'])
    assert np.array_equal(fc['edges'], kc['bins'])
    y = kc['y']
    d = float(np.max(np.abs(fc['k'] - y)) / np.max(np.abs(y)))
    print('state mode against the reference golden: largest deviation %.3e of max |k|' % d)
    assert d <= TOL_K_GOLDEN
    assert np.allclose(fc['cumulative'], np.cumsum(y, axis=1), rtol=0, atol=10 * TOL_K_GOLDEN * np.max(np.abs(y)) * y.shape[1])


# ---- band tables wider than one LDS tile (nk_band_tile / nk_band_pass: passes of Bt bands, k_spectral_reduce writing tile b0 at
# band offset b0) and modes in no band (-1: k_spectral's skip of b outside the tile)
# The upper bound of a tile, whatever else the kernels keep in LDS: nk_band_tile gives S x Bt bins of 28 B at most 64 KB.
def max_tile(S):
    return 65536 // (28 * S)


def holey_table(ct, nbands, kind, holes, seed):
    """kind 'frequency': band_map's bins of omega; 'permuted': band of mode m = perm(m) mod B, so that neighbouring modes fall in
    different tiles.  holes: about a third of the modes (drawn at random) in no band."""
    rng = np.random.default_rng(seed)
    M = ct['ph'].omega.size
    if kind == 'frequency':
        band, B = band_table(ct, nbands, kind)
    else:
        band, B = (rng.permutation(M) % nbands).astype(np.int32), nbands
    band = np.array(band, dtype=np.int32)
    if holes:
        band[rng.random(M) < 1.0 / 3.0] = -1
    return band, B


def slice100_case():
    from util import case_from_args
    argv = ['--geometry', 'box', '--dimensions', '2000', '200', '200', '--subvolumes', 'slice', '100', '0',
            '--bound_pos', 'relative', '0', '.5', '.5', '1', '.5', '.5', '--bound_cond', 'T', 'T', 'P',
            '--connect_pos', 'relative', '.5', '0', '.5', '.5', '1', '.5', '.5', '.5', '0', '.5', '.5', '1',
            '--bound_values', '302', '298', '--poscar_file', 'POSCAR', '--hdf_file', 'synthetic', '--temp_interp', 'linear',
            '--timestep', '1', '--energy_normal', 'mean', '--particles', 'total', '20000']
    return case_from_args(argv, 'Si')


@pytest.mark.parametrize('case,nbands,kind,holes', [('ttp', 250, 'frequency', False), ('ttp', 1000, 'permuted', True),
                                                    ('ttrrp', 250, 'permuted', True), ('slice100', 100, 'frequency', True)])
def test_band_tiles_against_oracle(case, nbands, kind, holes):
    """Several tiles of bands with a partial last one, bands dealt by a random permutation, a third of the modes in no band,
    and a film of 100 slices (a tile of a few bands): per band and step against the oracle's particles; the sum over the bands
    is the subvolume's count and flux less the particles in no band."""
    from util import rel_row, population_in_mesh, oracle_flux
    if case == 'slice100':
        ct = slice100_case()
        pos, mode, occ, counter = population_in_mesh(ct, 20000, seed=5)
    else:
        ct = case_tables(case)
        pos, mode, occ, counter = random_population(ct, 20000, seed=5)
    S = ct['centers'].shape[0]
    band, B = holey_table(ct, nbands, kind, holes, seed=nbands)
    assert B > max_tile(S)              # two tiles at least (b0 > 0) whatever else the kernels keep in LDS
    assert (band < 0).any() == holes
    sim = make_oracle_sim(ct, pos, mode, occ, counter, seed=3)
    eng = make_engine(ct, pos, mode, occ, counter, seed=3)
    same_event_rule(eng, sim)
    eng.set_bands(band, B)
    t = eng.step(20)
    assert list(t['band_steps']) == [9, 19]
    vg = np.asarray(ct['tables']['group_vel']).reshape(-1, 3)
    for s in range(20):
        sim.run_timestep()
        if (s + 1) % 10:
            continue
        r = list(t['band_steps']).index(s)
        F0, N0 = oracle_bands(sim, ct, band, B)
        assert np.array_equal(t['band_N'][r], N0), 'band counts differ at step %d' % s
        assert rel_row(t['band_F'][r], F0, tag='band_F', bound=TOL_BAND_F) <= TOL_BAND_F, 'band flux differs at step %d' % s
        # the particles in no band, from the oracle's: what the sums over the bands leave out
        n = sim.P.N
        out = band[sim.P.mode[:n]] < 0
        N_out = np.bincount(sim.P.sv[:n][out], minlength=S)
        F_out = np.zeros((S, 3))
        e = sim.P.energy[:n][out]
        v = vg[sim.P.mode[:n][out]]
        for d in range(3):
            np.add.at(F_out[:, d], sim.P.sv[:n][out], v[:, d] * e)
        assert np.array_equal(t['band_N'][r].sum(axis=1), t['N_sv'][s] - N_out)
        assert rel_row(t['band_F'][r].sum(axis=1), t['flux_raw'][s] - F_out, tag='band sum', bound=TOL_BAND_SUM) <= TOL_BAND_SUM
        assert rel_row(t['flux_raw'][s], oracle_flux(sim), tag='flux_raw', bound=TOL_BAND_SUM) <= TOL_BAND_SUM
    # the state mode on the same table against the host formula of test_state_mode_against_host
    F, N = eng.tally_bands_state()
    F0, N0 = state_on_host(eng, ct, band, B)
    assert np.array_equal(N, N0)
    assert rel_row(F, F0, tag='state band_F', bound=TOL_BAND_STATE) <= TOL_BAND_STATE


def state_on_host(eng, ct, band, B):
    p = eng.download()
    x, m, n = p['positions'], p['mode'].astype(int), p['occupation']
    S = ct['centers'].shape[0]
    sv = eng.classify(x)
    T = eng.eval('interp_T', x)
    om = ct['ph'].omega.ravel()[m]
    n0 = np.where(T > 0, eng.eval('occupation', T, m), 0.0)
    e = ct['ph'].hbar * om * (n - n0)
    v = np.asarray(ct['tables']['group_vel']).reshape(-1, 3)[m]
    keep = band[m] >= 0
    F0, N0 = np.zeros((S, B, 3)), np.zeros((S, B))
    for d in range(3):
        np.add.at(F0[:, :, d], (sv[keep], band[m][keep]), v[keep, d] * e[keep])
    np.add.at(N0, (sv[keep], band[m][keep]), 1.0)
    return F0, N0
