"""Replica groups (nk_group_create / engine.EngineGroup): R engines that hold the same problem under different seeds, stepped by
shared launches.  A member of a group does what it does alone: the same device functions, the same flags, the same order of the
column sums.  Needs a real MI355X: `pytest -m gpu`.

How equal is equal.  Measured on an MI355X (three members, 130 steps, with and without ids): the integers (N_sv, N_leaving,
N_emitted), T_sv, E_sv and every downloaded particle field of a group member are the solo run's bits.  E_raw, flux_raw,
res_energy and res_flux are not -- and neither are those of TWO SOLO RUNS of the same engine: a workgroup's four waves add
their terms to shared LDS bins with FP64 atomics, in whatever order they arrive.  Solo against solo: up to 2.2e-16 of the row's
largest |value| (E_raw 1220-1286 entries of 130 x 3 rows, flux_raw 177-196, res_energy 55-60, res_flux 774-786); group against
solo: up to 2.2e-16 (1262-1263, 188-192, 58-66, 766-812) -- the same scatter, so no expression was formed differently by the
compiler.  The comparisons below therefore hold the integers, T_sv, E_sv and the particles bit for bit (np.array_equal), and the
four atomically added sums to the project's tolerances for two runs that sum in different orders (util.RUN_TOL), recording the
deviations through util's recorder."""
import numpy as np
import pytest

from util import (case_tables, random_population, make_oracle_sim, make_engine, same_event_rule, oracle_row, assert_rows,
                  engine_row, ROW_KEYS, RUN_TOL)

pytestmark = pytest.mark.gpu

CALLS = (1, 7, 100, 22)          # 130 steps: step 100 is a contains_check step, thirteen heat-flux steps


def members(seeds, n=20000, case='ttp', track_ids=False, **kw):
    """One engine per seed, each with its own random population (20000 + 500 k particles, so that the members differ in size)."""
    ct = case_tables(case)
    out = []
    for k, s in enumerate(seeds):
        pos, mode, occ, counter = random_population(ct, n + 500 * k, seed=100 + s)
        out.append(make_engine(ct, pos, mode, occ, counter, seed=s, track_ids=track_ids, **kw))
    return out


def assert_same_rows(a, b, what):
    """Every row of a member's call `a` against the solo run's `b`: the counts, T_sv and E_sv bit for bit (measured equal, see the
    module docstring); the four sums added with FP64 LDS atomics to RUN_TOL."""
    for k in ROW_KEYS:
        assert a[k].shape == b[k].shape, '%s: %s has shape %r against %r' % (what, k, a[k].shape, b[k].shape)
    for k in ('N_sv', 'N_leaving', 'N_emitted', 'T_sv', 'E_sv'):
        assert np.array_equal(a[k], b[k]), '%s: %s differs (largest deviation %g)' % (what, k, np.max(np.abs(a[k] - b[k])))
    assert np.array_equal(np.isnan(a['flux_raw']), np.isnan(b['flux_raw'])), '%s: flux_raw on different steps' % what
    for s in range(b['N_sv'].shape[0]):
        try:
            assert_rows(a, s, engine_row(b, s), **RUN_TOL)
        except AssertionError as e:
            raise AssertionError('%s: %s' % (what, e))


def assert_same_particles(e1, e2, what):
    """The downloaded particles of two runs, every field bit for bit."""
    p, q = e1.download(), e2.download()
    for k in ('mode', 'facet', 'pid', 'positions', 'n_timesteps', 'occupation'):
        assert p[k].shape == q[k].shape and np.array_equal(p[k], q[k], equal_nan=True), '%s: downloaded %s differs' % (what, k)
    assert e1.get_step() == e2.get_step()


def group_of(engs):
    from nanokappa_amd.engine import EngineGroup
    return EngineGroup(engs)


def run_both(grouped, solo, calls=CALLS):
    """The same calls through a group of `grouped` and through Engine.step of every engine of `solo`; rows compared call by call."""
    g = group_of(grouped)
    for c, n in enumerate(calls):
        rows = g.step(n)
        assert len(rows) == len(grouped)
        for r, e in enumerate(solo):
            assert_same_rows(rows[r], e.step(n), 'member %d, call %d (%d steps)' % (r, c, n))
    for r, (a, b) in enumerate(zip(grouped, solo)):
        assert_same_particles(a, b, 'member %d' % r)
    return g


@pytest.mark.parametrize('variant', ['box', 'no_box', 'ids'])
def test_replica_equals_solo_run(variant, monkeypatch):
    """Three members with different seeds and populations, 130 steps in calls of 1, 7, 100 and 22, against three fresh engines
    doing the same calls through nk_step: every key of every row and the downloaded particles.  On the box store,
    on the cached store (NK_NO_BOX=1), and with particle ids tracked."""
    if variant == 'no_box':
        monkeypatch.setenv('NK_NO_BOX', '1')
    ids = variant == 'ids'
    seeds = (3, 4, 5)
    grouped, solo = members(seeds, track_ids=ids), members(seeds, track_ids=ids)
    assert int(grouped[0].timing()['box_store']) == (0 if variant == 'no_box' else 1)
    g = run_both(grouped, solo)
    info = g.info()
    assert info['R'] == 3 and info['steps'] == 130
    assert info['sweep_launches'] == 130 and info['tail_launches'] == 130
    assert info['halted'] == 0 and info['finished_alone'] == 0
    g.close()


def test_group_member_against_the_oracle():
    """One replica of a group of three against the CPU oracle over 25 steps, with the tolerances of the solo parity tests."""
    ct = case_tables('ttp')
    engs, sim = [], None
    for k, s in enumerate((7, 8, 9)):
        pos, mode, occ, counter = random_population(ct, 20000, seed=40 + s)
        engs.append(make_engine(ct, pos, mode, occ, counter, seed=s))
        if k == 1:
            sim = make_oracle_sim(ct, pos, mode, occ, counter, seed=s)
    same_event_rule(engs[1], sim)
    g = group_of(engs)
    done = 0
    for n in (5, 20):
        t = g.step(n)[1]
        for s in range(n):
            sim.run_timestep()
            assert_rows(t, s, oracle_row(sim), label=done + s)
        done += n
    g.close()


def test_membership_does_not_matter():
    """Seed s alone in a group of one, first of three and last of three: the same run."""
    ct = case_tables('ttp')

    def member(s, n=20000):
        pos, mode, occ, counter = random_population(ct, n, seed=100 + s)
        return make_engine(ct, pos, mode, occ, counter, seed=s, track_ids=False)

    runs = []
    for line_up in ((11,), (11, 12, 13), (12, 13, 11)):
        engs = [member(s) for s in line_up]
        g = group_of(engs)
        k = line_up.index(11)
        rows = [g.step(n)[k] for n in (3, 30)]
        runs.append((rows, engs[k], g, engs))
    for rows, eng, _, _ in runs[1:]:
        for a, b in zip(runs[0][0], rows):
            assert_same_rows(a, b, 'seed 11 in another group')
        assert_same_particles(runs[0][1], eng, 'seed 11 in another group')
    for _, _, g, _ in runs:
        g.close()


def test_a_members_store_grows(monkeypatch):
    """Member 1 has six times the entry rate and a store with hardly any head room (NK_TIGHT_STORE while it is built, as in
    test_store_grows_by_itself): it halts in the middle of a call while the others run on, is grown and finishes its steps
    alone.  All members equal their solo runs, every member delivers every row, and the group reports one halted member."""
    ct = case_tables('ttp')

    def build():
        out = []
        for k, s in enumerate((21, 22, 23)):
            pos, mode, occ, counter = random_population(ct, 20000, seed=9 + k)
            if k == 1:
                monkeypatch.setenv('NK_TIGHT_STORE', '1')
            out.append(make_engine(ct, pos, mode, occ, counter, seed=s, emit_scale=6.0 if k == 1 else 1.0))
            monkeypatch.delenv('NK_TIGHT_STORE', raising=False)
        return out

    grouped, solo = build(), build()
    slots0 = grouped[1].timing()['slots']
    g = run_both(grouped, solo, calls=(45, 45))
    assert solo[1].timing()['halts'] > 0 and solo[0].timing()['halts'] == 0 and solo[2].timing()['halts'] == 0
    tm = grouped[1].timing()
    assert tm['halts'] > 0 and tm['slots'] > slots0 and tm['live'] > slots0       # it did outgrow its first allocation
    assert grouped[0].timing()['halts'] == 0 and grouped[2].timing()['halts'] == 0
    info = g.info()
    assert info['halted'] == 1 and info['finished_alone'] == 1, info
    assert info['member_launches'] > 0
    g.close()


def test_launch_count_does_not_depend_on_R():
    """The property the feature exists for: over steps without a contains_check step, a group of four issues the launches of a
    group of one -- two per step -- and none for a single member."""
    counts = {}
    for R in (1, 4):
        engs = members(range(30, 30 + R))
        g = group_of(engs)
        g.step(3)                                  # step 0 is a contains_check step and needs a first emission per member
        i0 = g.info()
        g.step(60)
        g.step(2)
        i1 = g.info()
        counts[R] = (i1['sweep_launches'] - i0['sweep_launches'], i1['tail_launches'] - i0['tail_launches'])
        assert i1['member_launches'] == i0['member_launches'], 'R = %d: launches for single members' % R
        assert i1['steps'] - i0['steps'] == 62
        assert i1['grid_sweep'] > 0 and i1['grid_tail'] > 0
        g.close()
    assert counts[1] == counts[4] == (62, 62)


def test_hand_over_between_group_and_solo_steps():
    """Group steps, then nk_step on one member alone, then -- after the others have caught up -- a new group of all members: still
    the solo runs.  Destroying a group leaves its members usable."""
    from nanokappa_amd.engine import NkError
    seeds = (41, 42, 43)
    grouped, solo = members(seeds), members(seeds)
    rows_g = [[] for _ in seeds]
    rows_s = [[] for _ in seeds]
    g = group_of(grouped)
    for r, t in enumerate(g.step(13)):
        rows_g[r].append(t)
    rows_g[2].append(grouped[2].step(9))            # member 2 alone, the group still exists
    with pytest.raises(NkError) as e:               # ... and refuses to step members that are no longer at the same step
        g.step(1)
    assert e.value.code == -2 and 'member 2' in str(e.value) and 'step' in str(e.value)
    g.close()
    rows_g[0].append(grouped[0].step(9))            # usable after the group is gone
    rows_g[1].append(grouped[1].step(9))
    g = group_of(grouped)
    for r, t in enumerate(g.step(95)):              # across the contains_check of step 100
        rows_g[r].append(t)
    g.close()
    for r, e in enumerate(solo):
        for n in (13, 9, 95):
            rows_s[r].append(e.step(n))
    for r in range(3):
        for c, (a, b) in enumerate(zip(rows_g[r], rows_s[r])):
            assert_same_rows(a, b, 'member %d, call %d' % (r, c))
        assert_same_particles(grouped[r], solo[r], 'member %d' % r)


def test_refusals():
    """NK_ERR_ARG with a message that names the member and the reason; nothing is launched (the members have not moved)."""
    from nanokappa_amd.engine import EngineGroup, NkError
    good = members((51, 52))

    def refused(engs, *words):
        with pytest.raises(NkError) as e:
            EngineGroup(engs)
        assert e.value.code == -2, str(e.value)
        for w in words:
            assert w in str(e.value), '%r not in %r' % (w, str(e.value))
        for x in engs:
            assert x.get_step() == 0

    ct = case_tables('ttrrp')
    pos, mode, occ, counter = random_population(ct, 20000, seed=1)
    rough = make_engine(ct, pos, mode, occ, counter, seed=1)
    refused([good[0], rough], 'member 1', 'rough')
    banded = members((53,))[0]
    nb = 4
    banded.set_bands(np.arange(banded.M, dtype=np.int32) % nb, nb)
    refused([good[0], good[1], banded], 'member 2', 'band')
    refused([good[0], good[0]], 'member 1', 'twice')
    refused([], 'R = 0')
    ahead = members((54,))[0]
    ahead.step(2)
    with pytest.raises(NkError) as e:
        EngineGroup([good[0], ahead])
    assert e.value.code == -2 and 'member 1' in str(e.value) and 'step' in str(e.value)
    assert good[0].get_step() == 0 and ahead.get_step() == 2
    # the refused engines still work, alone and in a group
    g = EngineGroup(good)
    assert len(g.step(2)) == 2
    g.close()


# ------------------------------------------------------------------------------------------------- Ensemble (Population level)
def population_args(case, particles, seed, folder, extra=()):
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden'))
    import ref_harness_args as A
    from nanokappa_amd.argument_parser import initialise_parser
    args = initialise_parser().parse_args(A.argv_for(case, particles) + ['--seed', str(seed)] + list(extra))
    args.results_folder = str(folder) if folder else ''
    return args


def convergence_columns(path):
    """convergence.txt without its first column (the wall-clock time of the row)."""
    with open(path) as f:
        return [line.split(None, 1)[1] if not line.startswith('#') else line for line in f]


@pytest.mark.parametrize('case', ['ttp', 'ttrrp'])
def test_ensemble_equals_solo_populations(case, tmp_path):
    """R = 3 on a small box against three Populations run alone with the same seeds: every replica's convergence.txt byte for
    byte (but for the wall-clock column), ensemble.txt against NumPy's mean, std (ddof = 1) and standard error of the replicas'
    values.  'ttp' is grouped; 'ttrrp' (rough walls) runs ungrouped, gives the same files and says why."""
    import os
    from util import golden_material
    from nanokappa_amd.geometry import Geometry
    from nanokappa_amd.phonon import Phonon
    from nanokappa_amd.population import Population
    from nanokappa_amd.ensemble import Ensemble, replica_seeds, read_summary
    seeds = replica_seeds([301], [3])
    assert seeds == [301, 302, 303]
    nsteps, particles = 230, 20000
    ens_dir = tmp_path / 'ens'
    ens_dir.mkdir()
    args = population_args(case, particles, seeds[0], ens_dir)
    geo = Geometry(args)
    ph = Phonon(args, 0, material=golden_material())
    ens = Ensemble(args, geo, ph, seeds)
    if case == 'ttp':
        assert ens.grouped and ens.why_not is None
    else:
        assert not ens.grouped and 'rough' in ens.why_not and 'member 0' in ens.why_not
    ens.run(nsteps)
    assert ens.current_timestep == nsteps
    summary = ens.write_summary()
    if case == 'ttp':
        info = ens.group.info()
        assert info['steps'] == nsteps and info['sweep_launches'] == nsteps
    ens.close()
    solo = []
    for k, s in enumerate(seeds):
        d = tmp_path / ('solo_%d' % k)
        d.mkdir()
        a = population_args(case, particles, s, d)
        pop = Population(a, geo, ph)
        pop.run(nsteps, geo, ph)
        solo.append(pop)
        assert os.path.isdir(ens_dir / ('replica_%d' % k))
        got = convergence_columns(ens_dir / ('replica_%d' % k) / 'convergence.txt')
        want = convergence_columns(d / 'convergence.txt')
        assert len(got) == len(want) == 2 + nsteps // 10
        assert got == want, 'convergence.txt of replica %d differs from the solo run' % k
    # the statistics: NumPy on the replicas' own window means (what _Stats computes over the last n_mean convergence rows)
    kap = []
    for pop in ens.populations:
        pop.view.postprocess()
        kap.append(pop.view.mean_k)
    kap = np.array(kap)
    txt = read_summary(ens_dir / 'ensemble.txt')
    R = len(seeds)
    assert txt['kappa'].shape == (1, 3 + 2 * R)
    assert txt['kappa'][0, 0] == np.mean(kap) == summary['kappa']['mean'][0]
    assert txt['kappa'][0, 1] == np.std(kap, ddof=1)
    assert txt['kappa'][0, 2] == np.std(kap, ddof=1) / np.sqrt(R)
    assert np.array_equal(txt['kappa'][0, 3::2], kap)
    Tm = np.array([pop.view.mean_T for pop in ens.populations])
    assert np.array_equal(txt['T_sv'][:, 0], Tm.mean(axis=0)) and np.array_equal(txt['T_sv'][:, 1], Tm.std(axis=0, ddof=1))
    assert np.array_equal(txt['T_sv'][:, 2], Tm.std(axis=0, ddof=1) / np.sqrt(R))
    Pm = np.array([pop.view.mean_sv_phi for pop in ens.populations])
    assert np.array_equal(txt['phi'][:, 0], Pm.mean(axis=0)) and np.array_equal(txt['phi'][:, 1], Pm.std(axis=0, ddof=1))
    head = open(ens_dir / 'ensemble.txt').read().splitlines()[:2]
    assert head[0].startswith('# replicas 3') and head[1].startswith('# grouped ' + ('yes' if case == 'ttp' else 'no: '))
    for pop in solo + ens.populations:
        pop.engine.close()


def test_config1_at_size():
    """BASELINE config 1 at its own size, eight replicas of 1e5 particles, 200 steps through a group: particle balance and census
    of every replica (as tests/test_gpu_fullsize.py), and replica 0 against its solo run."""
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
    import bench
    from nanokappa_amd import synthetic
    from nanokappa_amd.argument_parser import initialise_parser
    from nanokappa_amd.geometry import Geometry
    from nanokappa_amd.phonon import Phonon
    from nanokappa_amd.population import Population
    total, nsteps, R = 100000, 200, 8
    argv, species, _ = bench.config_argv('c2', total, 200.0)
    ph = Phonon(initialise_parser().parse_args(argv), 0, material=synthetic.make_material(31, species, temperatures=np.arange(200.0, 401.0, 10.0)))
    geo = None

    def population(seed):
        nonlocal geo
        args = initialise_parser().parse_args(argv + ['--seed', str(seed), '--device', '0'])
        args.results_folder = ''
        if geo is None:
            geo = bench.quiet(Geometry, args)
        return bench.quiet(Population, args, geo, ph, None, None)

    pops = [population(2025 + k) for k in range(R)]
    n0 = [int(p.N_p) for p in pops]
    assert n0 == [total] * R
    g = group_of([p.engine for p in pops])
    ts = g.step(nsteps)
    info = g.info()
    assert info['sweep_launches'] == nsteps and info['tail_launches'] == nsteps and info['R'] == R
    for k, t in enumerate(ts):
        N = t['N_sv'].sum(axis=1)
        prev = np.concatenate(([n0[k]], N[:-1]))
        assert np.array_equal(N - prev, t['N_emitted'] - t['N_leaving'].sum(axis=1)), 'particle balance of replica %d' % k
        assert t['N_emitted'].min() > 0 and t['N_leaving'].min() > 0
        assert int(N[-1]) == int(pops[k].engine.timing()['live']), 'census of replica %d against its store' % k
        assert np.all(np.isfinite(t['T_sv'])) and t['T_sv'].min() > 290.0 and t['T_sv'].max() < 310.0
    solo = population(2025)
    assert_same_rows(ts[0], solo.engine.step(nsteps), 'replica 0')
    assert_same_particles(pops[0].engine, solo.engine, 'replica 0')
    assert not np.array_equal(ts[0]['N_sv'], ts[1]['N_sv'])         # the replicas are different runs
    g.close()


def test_ungrouped_ensemble_with_a_tally_writes_every_replicas_files(tmp_path):
    """--spectral_bands is outside the grouped path: the ensemble steps its populations one after another, says why, and every
    replica still writes what a run of its own writes at its end -- k_contribution.txt beside the final state -- with the
    numbers of a solo Population under the same seed."""
    import os
    from util import golden_material
    from nanokappa_amd.geometry import Geometry
    from nanokappa_amd.phonon import Phonon
    from nanokappa_amd.population import Population
    from nanokappa_amd.ensemble import Ensemble
    extra = ['--spectral_bands', '6', 'frequency']
    seeds, nsteps, particles = [311, 312], 120, 20000
    ens_dir = tmp_path / 'ens'
    ens_dir.mkdir()
    args = population_args('ttp', particles, seeds[0], ens_dir, extra)
    geo = Geometry(args)
    ph = Phonon(args, 0, material=golden_material())
    ens = Ensemble(args, geo, ph, seeds)
    assert not ens.grouped and 'member 0' in ens.why_not and 'band' in ens.why_not
    ens.run(nsteps)
    ens.write_final_state()
    ens.write_summary()
    ens.close()
    assert os.path.exists(ens_dir / 'ensemble.txt')
    for k, s in enumerate(seeds):
        d = tmp_path / ('solo_%d' % k)
        d.mkdir()
        pop = Population(population_args('ttp', particles, s, d, extra), geo, ph)
        pop.run(nsteps, geo, ph)
        pop.finish_run(geo)
        pop.engine.close()
        rep = ens_dir / ('replica_%d' % k)
        want = sorted(f for f in os.listdir(d))
        got = sorted(f for f in os.listdir(rep))
        assert 'k_contribution.txt' in want and got == want, (got, want)
        assert convergence_columns(rep / 'convergence.txt') == convergence_columns(d / 'convergence.txt')
        a, b = np.loadtxt(rep / 'k_contribution.txt'), np.loadtxt(d / 'k_contribution.txt')
        assert a.shape == b.shape and a.size > 0
        # (printed with nine digits; the band sums are added with FP64 atomics, 1e-16 apart between two runs)
        assert np.allclose(a, b, rtol=1e-9, atol=1e-9 * np.nanmax(np.abs(b)), equal_nan=True)
    for p in ens.populations:
        p.engine.close()
