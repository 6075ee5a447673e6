"""The oracle's tally row of one step (util.oracle_row), which the GPU parity tests hold every row of Engine.step against: its
flux_raw is the oracle's own heat flux with the normalisation undone, its per-step reservoir tallies add up to the oracle's
running sums, N_emitted closes the particle balance, and the row does not depend on which event rule the oracle runs (the
reference's cached n_timesteps or the box rule).  CPU only."""
import numpy as np
import pytest

from util import case_tables, random_population, make_oracle_sim, oracle_row, ROW_KEYS


def flux_of_oracle(sim):
    """sim.flux (nko_heat_flux: W m^-2, normalised by active modes / N_sv) back to the engine's unnormalised flux_raw."""
    eVpsa2_in_Wm2 = 1.602176634e-19 / (1e-12 * (1e-10 * 1e-10))
    return sim.flux * sim.N_sv[:, None] / sim.mat.active_modes * sim.mat.QV / eVpsa2_in_Wm2


@pytest.mark.parametrize('case,gen', [('ttp', 0), ('ttrrp', 0), ('ttp', 2)])
def test_oracle_row_against_the_oracles_own_tallies(case, gen):
    ct = case_tables(case)
    pos, mode, occ, counter = random_population(ct, 20000, seed=5)
    sim = make_oracle_sim(ct, pos, mode, occ, counter, seed=21, gen=gen)
    res_e, res_f, flux_steps = np.zeros(2), np.zeros((2, 3)), 0
    prev_leaving = None
    for s in range(40):
        n0 = sim.P.N
        sim.run_timestep()
        row = oracle_row(sim)
        assert set(row) == set(ROW_KEYS)
        assert row['flux_raw'].shape == (20, 3) and row['res_flux'].shape == (2, 3) and row['N_leaving'].shape == (2,)
        # particle balance: what came in minus what left through the reservoirs
        assert sim.P.N == n0 + row['N_emitted'] - row['N_leaving'].sum(), 'step %d' % s
        assert row['N_emitted'] > 0
        if gen == 2 and prev_leaving is not None:
            assert row['N_emitted'] == prev_leaving.sum()
        prev_leaving = row['N_leaving']
        res_e += row['res_energy']
        res_f += row['res_flux']
        if (s + 1) % 10 == 0:
            flux_steps += 1
            F, F0 = row['flux_raw'], flux_of_oracle(sim)
            assert np.abs(F - F0).max() <= 1e-13 * np.abs(F0).max(), 'step %d' % s
            assert np.array_equal(row['N_sv'], sim.N_sv)
        else:
            assert np.isnan(row['flux_raw']).all()
    assert flux_steps == 4
    # the steps' shares add up to the oracle's running sums
    assert np.abs(res_e - sim.res_energy[:2]).max() <= 1e-12 * np.abs(sim.res_energy[:2]).max()
    assert np.abs(res_f - sim.res_flux[:2]).max() <= 1e-12 * np.abs(sim.res_flux[:2]).max()


@pytest.mark.parametrize('case', ['ttp', 'ttrrp'])
def test_oracle_rows_equal_under_both_event_rules(case):
    """The pattern of test_oracle_box_rule: the same events under both rules, so the same counts at every step and reals equal
    to the rounding of the drift, across a contains_check (step 100).  E_raw adds energies relative to the subvolume's own
    temperature, which nearly cancel (measured 1.2e-12 of the row's largest |value|, 'ttrrp'); the rest below 3e-14."""
    ct = case_tables(case)
    pos, mode, occ, counter = random_population(ct, 20000, seed=7)
    a = make_oracle_sim(ct, pos, mode, occ, counter, seed=9, box=False)
    b = make_oracle_sim(ct, pos, mode, occ, counter, seed=9, box='auto')
    assert a.p.box == 0 and b.p.box == 1
    for s in range(130):
        a.run_timestep()
        b.run_timestep()
        ra, rb = oracle_row(a), oracle_row(b)
        for k in ('N_sv', 'N_leaving', 'N_emitted'):
            assert np.array_equal(ra[k], rb[k]), '%s, step %d' % (k, s)
        assert np.array_equal(np.isnan(ra['flux_raw']), np.isnan(rb['flux_raw']))
        for k in ('E_raw', 'T_sv', 'E_sv', 'flux_raw', 'res_energy', 'res_flux'):
            x, y = np.nan_to_num(ra[k]), np.nan_to_num(rb[k])
            bound = 1e-11 if k == 'E_raw' else 3e-13
            assert np.abs(x - y).max() <= bound * max(np.abs(y).max(), 1e-300), '%s, step %d' % (k, s)
