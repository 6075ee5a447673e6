"""The engine away from dt = 1 ps and from lifetimes of eight steps and more.  Needs a real MI355X: `pytest -m gpu`.

Every other GPU test runs dt = 1 on the synthetic Si, whose shortest lifetime at 300 K is 13.98 ps: dt is only ever multiplied in
as 1.0, and nk_relax's exponential is always the short series (no lane of any wave has dt / tau >= 1/8).  A setting here is
(dt, v_scale, tau_scale), applied by util.scaled_case:

  U = (1, 1, 1)      what every other test runs
  A = (2, 1/2, 2)    the same physics in another time unit: v dt, dt / tau, t_hit / dt and enter_prob are the same doubles, so the
                     run must reproduce U step for step; only flux_raw = sum v e halves (tests/test_oracle_timestep.py holds the
                     oracle to that, bit for bit)
  B = (2, 1, 1)      a real 2 ps step: twice the flight per step, 7.8 % of the modes over the threshold
  C = (1, 1, 1/32)   91 % of the modes on the general exponential, dt / tau up to 2.29
  D = (1, 1, 1/2)    on a population drawn from the modes under the threshold plus 1 % from those over it: waves without and
                     with an over-threshold lane in the same launch, so both sides of nk_relax's wave vote run

All runs: 30 000 particles, 25 steps, seed 42, as test_gpu_parity.test_multistep_vs_oracle; tolerances are the project's (util.TOL_*,
measured at dt = 1): B, C and D stay inside them (profiles/timestep_parity_margins.txt)."""
import os
import sys

import numpy as np
import pytest

from util import (case_tables, case_from_args, scaled_case, random_population, population_in_mesh, make_oracle_sim, make_engine,
                  same_event_rule, oracle_row, assert_rows, engine_row, allclose, rel_err, rel_row, golden_material, RUN_TOL,
                  TOL_T, TOL_X, TOL_X_LONG, TOL_NTS, TOL_OCC, TOL_ROW_RES, TOL_RUN_FLUX)

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden'))

N, NSTEPS, SEED = 30000, 25, 42
SETTINGS = dict(U=(1.0, 1.0, 1.0), A=(2.0, 0.5, 2.0), B=(2.0, 1.0, 1.0), C=(1.0, 1.0, 1.0 / 32), D=(1.0, 1.0, 0.5))

_CASES = {}


def base_case(name):
    """The unscaled case and its starting population, built once per module."""
    if name not in _CASES:
        if name in ('ttp', 'ttrrp'):
            ct = case_tables(name)
            pop = random_population(ct, N, seed=5)
        else:
            from test_gpu_parity import EXTRA_CASES, COMMON_ARGS
            argv, species = EXTRA_CASES[name]
            ct = case_from_args(argv + COMMON_ARGS, species)
            pop = population_in_mesh(ct, N, seed=8 if name == 'wire16' else 21)
        _CASES[name] = (ct, pop)
    return _CASES[name]


def mode_classes(ct, dt=1.0):
    """(under, over): the active modes whose dt / tau is below / at least 1/8 everywhere between 290 and 310 K (the
    temperatures of these runs lie between 297 and 303 K; lifetimes are interpolated linearly between the grid's rows)."""
    tb = ct['tables']
    rows = np.nonzero((tb['T_grid'] >= 290.0) & (tb['T_grid'] <= 310.0))[0]
    assert rows.shape[0] == 3
    tau = tb['lifetime'].reshape(tb['lifetime'].shape[0], -1)[rows]
    active = ~ct['ph'].inactive_modes_mask.ravel() & (tau.min(axis=0) > 0)
    return np.nonzero(active & (tau.min(axis=0) > 8.0 * dt))[0], np.nonzero(active & (tau.max(axis=0) < 8.0 * dt))[0]


def compare_particles(p, sim, tol_x, label):
    n = sim.P.N
    assert p['pid'].shape[0] == n
    o1, o2 = np.argsort(p['pid']), np.argsort(sim.P.pid[:n])
    assert np.array_equal(p['pid'][o1], sim.P.pid[:n][o2])
    assert np.array_equal(p['mode'][o1], sim.P.mode[:n][o2])
    assert np.array_equal(p['facet'][o1], sim.P.facet[:n][o2])
    assert allclose(p['positions'][o1], sim.P.pos[:n][o2], rtol=0, atol=tol_x, depth=2, tag=label + ' positions')
    assert allclose(p['n_timesteps'][o1], sim.P.n_ts[:n][o2], rtol=0, atol=TOL_NTS, depth=2, tag=label + ' n_timesteps')
    assert rel_err(p['occupation'][o1], sim.P.occ[:n][o2], depth=2, tag=label + ' occupation', bound=TOL_OCC) < TOL_OCC


# ------------------------------------------------------------------------------------------------ 1. the unit change, engine
@pytest.mark.parametrize('path', ['ttp-box', 'ttp-cached', 'ttrrp'])
def test_engine_is_invariant_under_the_time_unit(path, monkeypatch):
    """Engine at A against engine at U.  The arithmetic is the same doubles: counts, ids, modes, facets, positions, n_timesteps,
    occupations, T_sv and E_sv bit for bit; E_raw, res_energy, res_flux and 2 x flux_raw are added with FP64 LDS atomics in
    arrival order and differ between two identical runs (DESIGN): the tolerances of two runs (util.RUN_TOL)."""
    if path == 'ttp-cached':
        monkeypatch.setenv('NK_NO_BOX', '1')
    ct, (pos, mode, occ, counter) = base_case(path.split('-')[0])
    runs = {}
    for key in ('U', 'A'):
        dt, vs, ts = SETTINGS[key]
        eng = make_engine(scaled_case(ct, dt, vs, ts), pos, mode, occ, counter, seed=SEED, dt=dt)
        if path != 'ttrrp':
            assert int(eng.timing()['box_store']) == (1 if path == 'ttp-box' else 0)
        t = eng.step(NSTEPS)
        p = eng.download()
        eng.close()
        runs[key] = (t, p)
    (tu, pu), (ta, pa) = runs['U'], runs['A']
    assert tu['N_emitted'].sum() > 0 and tu['N_leaving'].sum() > 0
    for k in ('N_sv', 'N_leaving', 'N_emitted', 'T_sv', 'E_sv'):
        assert np.array_equal(ta[k], tu[k]), '%s differs (largest deviation %g)' % (k, np.max(np.abs(ta[k] - tu[k])))
    ta2 = dict(ta)
    ta2['flux_raw'] = ta['flux_raw'] * 2.0
    for s in range(NSTEPS):
        assert_rows(ta2, s, engine_row(tu, s), **RUN_TOL)
    o1, o2 = np.argsort(pa['pid']), np.argsort(pu['pid'])
    for k in ('pid', 'mode', 'facet', 'positions', 'n_timesteps', 'occupation'):
        assert np.array_equal(pa[k][o1], pu[k][o2]), '%s differs (largest deviation %g)' % (k, np.max(np.abs(pa[k][o1].astype(float) - pu[k][o2].astype(float))))


# --------------------------------------------------------------------------------- 2. engine against oracle at B, C and D
PATHS = ['ttp-box', 'ttp-cached', 'ttp-resident', 'ttrrp', 'wire16', 'wire72', 'ttp-group']


def restricted_population(ct, share=0.01, seed=5):
    """Setting D's population: the modes under the threshold (at tau_scale 1/2: a lifetime of more than 16 ps), and with
    probability `share` one of those over it."""
    pos, mode, occ, counter = random_population(ct, N, seed=seed)
    under, over = mode_classes(scaled_case(ct, 1.0, 1.0, 0.5))
    rng = np.random.default_rng(seed + 1000)
    pick = rng.random(N) < share
    mode = np.where(pick, over[rng.integers(0, over.shape[0], N)], under[rng.integers(0, under.shape[0], N)]).astype(np.int32)
    ph = ct['ph']
    occ = ph.calculate_occupation(298.0, ph.omega.ravel()[mode])
    return pos, mode, occ, counter


def wave_census(eng, p, under, over):
    """(pure, mixed): the 64-particle tiles of the store as downloaded -- the segments one after another, a wave takes 64
    consecutive particles of one segment -- that hold only under-threshold modes / at least one over- and one under-threshold
    mode."""
    seg_of_mode, nseg = eng.mode_segments()
    seg = seg_of_mode[p['mode']]
    assert np.all(np.diff(seg) >= 0)                        # the download is in segment order
    is_over, is_under = np.isin(p['mode'], over), np.isin(p['mode'], under)
    first = np.searchsorted(seg, np.arange(nseg), side='left')
    tile = (np.arange(seg.shape[0]) - first[seg]) // 64
    key = seg.astype(np.int64) * (1 << 20) + tile
    _, inv = np.unique(key, return_inverse=True)
    n_over = np.bincount(inv, weights=is_over)
    n_under = np.bincount(inv, weights=is_under)
    n_all = np.bincount(inv)
    return int(np.sum((n_under == n_all))), int(np.sum((n_over > 0) & (n_under > 0)))


@pytest.mark.parametrize('path,setting', [(p, s) for s in ('B', 'C') for p in PATHS] + [('ttp-box', 'D'), ('ttp-cached', 'D')])
def test_engine_vs_oracle_away_from_unit_timestep(path, setting, monkeypatch):
    """Same seed, same counter-based random numbers: engine and oracle make the same decisions at a 2 ps step (B), with 91 % of
    the modes on the general exponential (C) and with both exponentials in one launch (D).  Every stepping path: box store, cached
    store, resident kernel, rough box, a faceted wire in LDS, a wire of 288 faces (split sweep, k_events), and a member of a
    replica group of three.  The download flushes the deferred relaxation through k_relax."""
    name = path.split('-')[0]
    if path == 'ttp-cached':
        monkeypatch.setenv('NK_NO_BOX', '1')
    if path == 'ttp-resident':
        monkeypatch.setenv('NK_RESIDENT', '1')
    ct0, pop = base_case(name)
    dt, vs, ts = SETTINGS[setting]
    ct = scaled_case(ct0, dt, vs, ts)
    if setting == 'D':
        pop = restricted_population(ct0)
    pos, mode, occ, counter = pop
    wire = name.startswith('wire')
    sim = make_oracle_sim(ct, pos, mode, occ, counter, seed=SEED, cap=200000, dt=dt)
    eng = make_engine(ct, pos, mode, occ, counter, seed=SEED, dt=dt)
    rule = same_event_rule(eng, sim)
    if name == 'ttp':
        assert rule == (0 if path == 'ttp-cached' else 1)
    group, others = None, []
    if path == 'ttp-group':
        from nanokappa_amd.engine import EngineGroup
        for k in (1, 2):
            q = random_population(ct0, N + 500 * k, seed=5 + k)
            others.append(make_engine(ct, *q, seed=SEED + k, dt=dt))
        group = EngineGroup([others[0], eng, others[1]])
        t = group.step(NSTEPS)[1]
    else:
        t = eng.step(NSTEPS)
    if name == 'ttp' and group is None:
        assert eng.timing()['emit_fused'] == (2 if path == 'ttp-resident' else 1)
    for s in range(NSTEPS):
        sim.run_timestep()
        assert_rows(t, s, oracle_row(sim))
    assert t['N_emitted'].sum() > 0 and t['N_leaving'].sum() > 0
    p = eng.download()
    compare_particles(p, sim, TOL_X_LONG if wire else TOL_X, setting + (' wire' if wire else ' box'))
    # the accumulated reservoir balance: every step's row is within TOL_ROW_RES of its largest |value| (assert_rows), so is their
    # sum (a reservoir whose inflow and outflow nearly cancel has no digits of its own to compare)
    assert rel_row(t['res_energy'].sum(axis=0), sim.res_energy[:2], tag='res_energy sum', bound=TOL_ROW_RES) <= TOL_ROW_RES
    if setting == 'D':
        under, over = mode_classes(ct)
        pure, mixed = wave_census(eng, p, under, over)
        print('setting D, %s: %d pure and %d mixed waves' % (path, pure, mixed))
        assert pure >= 1 and mixed >= 1, 'only one side of the wave vote ran: %d pure, %d mixed waves' % (pure, mixed)
    elif name == 'ttp':       # B and C: the general exponential runs -- some wave holds a mode with dt / tau >= 1/8
        under, over = mode_classes(ct, dt)
        assert np.isin(p['mode'], over).sum() > (500 if setting == 'B' else 15000)
    if group is not None:
        group.close()
    for e in [eng] + others:
        e.close()


# ------------------------------------------------------------------------------------------------------ 4. Population level
def test_population_under_the_time_unit():
    """Population with --timestep 2 on the material with halved group velocities and halved scattering rates against --timestep 1
    on the plain material, same seed: dt through enter_probability, set_params, calculate_kappa and the step clock.  The rows'
    temperatures and particle counts are the same; heat flux and kappa of the scaled run, times 2, are the plain run's."""
    from nanokappa_amd.argument_parser import initialise_parser
    from nanokappa_amd.geometry import Geometry
    from nanokappa_amd.phonon import Phonon
    from nanokappa_amd.population import Population
    import ref_harness_args as A
    rows = {}
    for key, dt, scale in (('U', '1', 1.0), ('A', '2', 0.5)):
        argv = A.argv_for('ttp', 20000) + ['--seed', '42']
        argv[argv.index('--timestep') + 1] = dt
        args = initialise_parser().parse_args(argv)
        args.results_folder = ''
        mat = golden_material()
        mat['group_vel'] = mat['group_vel'] * scale
        mat['gamma'] = np.where(mat['gamma'] > 0, mat['gamma'] * scale, mat['gamma'])
        geo = Geometry(args)
        ph = Phonon(args, 0, material=mat)
        pop = Population(args, geo, ph)
        rec = []
        for _ in range(4):                                                  # 40 steps, a convergence row every 10
            pop.run(10, geo, ph)
            rec.append(dict(step=pop.current_timestep, N_p=pop.N_p, kappa=pop.kappa, T=np.array(pop.subvol_temperature),
                            flux=np.array(pop.subvol_heat_flux), N_sv=np.array(pop.subvol_N_p), kappa_sv=np.array(pop.subvol_kappa)))
        pop.engine.close()
        rows[key] = rec
    for u, a in zip(rows['U'], rows['A']):
        assert u['step'] == a['step'] and u['N_p'] == a['N_p'] and np.array_equal(u['N_sv'], a['N_sv'])
        assert allclose(a['T'], u['T'], rtol=0, atol=TOL_T, tag='T_sv')
        assert np.abs(u['flux']).max() > 0 and np.isfinite(u['kappa']) and u['kappa'] != 0
        assert rel_row(2.0 * a['flux'], u['flux'], tag='heat flux', bound=TOL_RUN_FLUX) <= TOL_RUN_FLUX
        assert rel_row(2.0 * a['kappa_sv'], u['kappa_sv'], tag='subvolume kappa', bound=TOL_RUN_FLUX) <= TOL_RUN_FLUX
        assert rel_row([2.0 * a['kappa']], [u['kappa']], tag='kappa', bound=TOL_RUN_FLUX) <= TOL_RUN_FLUX
