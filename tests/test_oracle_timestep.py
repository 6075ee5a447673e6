"""The CPU oracle under a change of the time unit.  Every test and golden runs dt = 1, so a forgotten dt, or one applied twice,
would go unseen.  A setting (dt, v_scale, tau_scale) = (2^k, 2^-k, 2^k) is the same physics in another time unit: v dt,
dt / tau, t_hit / dt and enter_prob = max(0, v.n) dt / thickness are the same doubles (the scales are powers of two), so the run
must reproduce (1, 1, 1) bit for bit.  Only flux_raw = sum v e carries a velocity and scales by v_scale; res_flux does not
change: its terms are e / (v.n) times v (Population.py:1602).  All three reservoir generators: 'constant', 'fixed_rate' and
'one_to_one' (Population.py:408-489) are unit-free in this sense -- their entry times are fractions of dt."""
import numpy as np
import pytest

from util import case_tables, scaled_case, random_population, make_oracle_sim, oracle_row, ROW_KEYS

N, NSTEPS, CAP = 30000, 25, 200000
SETTINGS = [(2.0, 0.5, 2.0), (4.0, 0.25, 4.0)]
CASES = [('ttp', 0), ('ttrrp', 0), ('ttp', 1), ('ttp', 2)]       # generators 1 fixed_rate, 2 one_to_one (Population.py:408-489)

_RUNS = {}


def run(case, gen, setting):
    """(rows of every step with flux_raw on every step, final particles); computed once per (case, generator, setting)."""
    key = (case, gen, setting)
    if key not in _RUNS:
        dt, vs, ts = setting
        ct = case_tables(case)
        pos, mode, occ, counter = random_population(ct, N, seed=5)
        sim = make_oracle_sim(scaled_case(ct, dt, vs, ts), pos, mode, occ, counter, seed=42, cap=CAP, gen=gen, dt=dt)
        rows = []
        for s in range(NSTEPS):
            sim.run_timestep()
            rows.append(oracle_row(sim, flux_every=1))
        n = sim.P.N
        P = sim.P
        final = dict(pid=P.pid[:n].copy(), mode=P.mode[:n].copy(), facet=P.facet[:n].copy(), pos=P.pos[:n].copy(),
                     occ=P.occ[:n].copy(), n_ts=P.n_ts[:n].copy())
        _RUNS[key] = (rows, final)
    return _RUNS[key]


@pytest.mark.parametrize('setting', SETTINGS, ids=['dt2', 'dt4'])
@pytest.mark.parametrize('case,gen', CASES, ids=['ttp', 'ttrrp', 'ttp-fixed_rate', 'ttp-one_to_one'])
def test_oracle_is_invariant_under_the_time_unit(case, gen, setting):
    rows0, p0 = run(case, gen, (1.0, 1.0, 1.0))
    rows1, p1 = run(case, gen, setting)
    assert sum(r['N_emitted'] for r in rows0) > 0 and sum(r['N_leaving'].sum() for r in rows0) > 0
    for s in range(NSTEPS):
        for k in ROW_KEYS:
            if k != 'flux_raw':
                assert np.array_equal(rows1[s][k], rows0[s][k]), '%s differs at step %d' % (k, s)
        assert np.all(np.isfinite(rows0[s]['flux_raw']))
        assert np.array_equal(rows1[s]['flux_raw'], rows0[s]['flux_raw'] * setting[1]), 'flux_raw differs at step %d' % s
    for k in ('pid', 'mode', 'facet', 'pos', 'occ', 'n_ts'):
        assert np.array_equal(p1[k], p0[k]), k
