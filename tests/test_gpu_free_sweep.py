"""Free-path sweeps on the GPU (Engine.free_path_columns; k_free_columns): every column of a K-column call against the single
call (Engine.free_paths; k_free_paths) with that column's lifetimes, as bytes; against the CPU restatement
(tests/free_path_cases.py) with each column's lifetimes; the closed form and the invariant per column; non-interference with
the steps; the refusals; Population.free_path_sweep and --free_path_sweep.

The cases are free_path_cases.PARITY's 'ttp', 'ttrrp_k' and 'wire72' with ONE fixed set of five columns (columns())."""
import os
import sys

import numpy as np
import pytest

import free_path_cases as FC
from util import allclose, rel_err, random_population, make_engine
from test_free_path_host import invariant, L_BOX
from test_gpu_free_path import fp_engine, wave_sum, TOL_RAY_D, TOL_RAY_T, TOL_MODE_W

pytestmark = pytest.mark.gpu

SUMS = ('D', 'D2', 'T', 'hits', 'p_res', 'p_wall', 'w_left', 'p_int')
RAYS = ('ray_D', 'ray_T', 'ray_segments', 'ray_end')
COUNTS = ('casts', 'missed', 'capped')
CASES = ('ttp', 'ttrrp_k', 'wire72')


def columns(ct, modes):
    """The five columns of tau = lifetimes(300 K): tau (the plain call), tau / 2 (a scale), tau 2^-12 (dies after the first
    segments while the others fly on), tau 2^10 (runs into the cap on 'ttp'), tau with every third listed mode set to 0 (a column
    that never starts there; on the rough cases, reflections into a dead mode)."""
    tau = FC.lifetimes(ct)
    dead = tau.copy()
    dead[np.asarray(modes)[::3]] = 0.0
    return np.stack([tau, tau / 2.0, np.ldexp(tau, -12), np.ldexp(tau, 10), dead])


def call_args(name):
    p = FC.PARITY[name]
    ct = FC.case(p['case'])
    ref = FC.parity_run(name)
    return ct, ref, dict(n=p['n'], modes=ref['modes'], max_segments=p['max_segments'], x0=ref['ray_x0'], seed=p['seed'], rays=True)


def device_runs(name):
    """The five-column call and the five single calls of a case, on one engine (shared by the tests; not to be modified)."""
    def make():
        ct, ref, kw = call_args(name)
        taus = columns(ct, ref['modes'])
        eng = fp_engine(ct, seed=99)
        cols = eng.free_path_columns(taus, **kw)
        singles = [eng.free_paths(t, **kw) for t in taus]
        eng.close()
        return ct, taus, cols, singles
    return FC.cached(('free_sweep', 'device', name), make)


def assert_column_is_single(cols, c, single, label):
    for k in SUMS + RAYS:
        assert np.asarray(cols[k][c]).tobytes() == np.asarray(single[k]).tobytes(), '%s: column %d differs from the single call in %s' % (label, c, k)
    for k in COUNTS:
        assert int(cols[k][c]) == single['report'][k], (label, c, k)
    assert np.array_equal(cols['ray_x0'], single['ray_x0']) and np.array_equal(cols['modes'], single['modes'])


@pytest.mark.parametrize('name', CASES)
def test_columns_equal_single_calls(name):
    """Every column of the five-column call equals Engine.free_paths with that column's lifetimes on the same list, byte for byte:
    the rows, the per-ray D / T / segments / end, the per-column counts.  The casts actually made are those of the longest-lived
    column of every ray: never more than the columns' sum, never fewer than the largest column's."""
    ct, taus, cols, singles = device_runs(name)
    assert cols['columns'] == 5 and cols['D'].shape == (5,) + singles[0]['D'].shape and cols['ray_T'].shape == (5,) + singles[0]['ray_T'].shape
    for c in range(5):
        assert_column_is_single(cols, c, singles[c], name)
    rep = cols['report']
    assert rep['geometry_mode'] == (2 if name == 'wire72' else 1) and rep['n_columns'] == 5 and rep['launches'] == 1 and rep['tile'] >= 5
    assert rep['casts_shared'] == int(cols['ray_segments'].max(axis=0).sum())
    assert cols['casts'].max() <= rep['casts_shared'] <= cols['casts'].sum()
    # what the columns are there for
    seg = cols['ray_segments']
    assert np.all(seg[2] <= seg[3]) and np.all(seg[1] <= seg[0])
    if name != 'wire72':                                                         # (every ray of the wire ends at its first hit)
        assert (seg[2] < seg[0]).any()                                           # the short column dies while the others fly on
    dead = np.arange(seg.shape[1]) % 3 == 0
    assert np.all(seg[4][dead] == 0) and np.all(cols['p_int'][4][dead] == cols['n']) and np.all(cols['T'][4][dead] == 0)
    if name == 'ttp':
        assert cols['capped'][3] > cols['capped'][0] > 1000 and (cols['ray_end'][3] == 4).any()


def test_one_column_and_one_more_than_the_tile():
    """K = 1 (the instantiation without a tile), and K = tile + 1: the last column is flown by a second launch that repeats the
    casts, and equals its single call like the others."""
    name = 'ttrrp_k'
    ct, taus, cols, singles = device_runs(name)
    _, ref, kw = call_args(name)
    eng = fp_engine(ct, seed=3)
    one = eng.free_path_columns(taus[:1], **kw)
    assert_column_is_single(one, 0, singles[0], 'K = 1')
    assert one['report']['casts_shared'] == singles[0]['report']['casts'] == int(one['casts'][0]) and one['report']['launches'] == 1
    tile = cols['report']['tile']
    assert 1 <= tile < 32
    many = np.stack([taus[c % 5] for c in range(tile + 1)])
    got = eng.free_path_columns(many, **kw)
    assert got['report']['launches'] == 2 and got['columns'] == tile + 1
    for c in range(tile + 1):
        assert_column_is_single(got, c, singles[c % 5], 'K = tile + 1')
    first = int(got['ray_segments'][:tile].max(axis=0).sum())
    assert got['report']['casts_shared'] == first + int(got['casts'][tile])
    # reflections into a dead mode: with the fixed columns no ray of this case is reflected into one of the modes the fifth column
    # sets to 0, so a column that lives on the listed modes only -- every specular reflection out of the list ends it (code 0)
    # while the first column goes on
    only = np.zeros_like(taus[0])
    only[ref['modes']] = taus[0][ref['modes']]
    pair = eng.free_path_columns(np.stack([taus[0], only]), **kw)
    assert_column_is_single(pair, 0, singles[0], 'dead outside the list')
    assert_column_is_single(pair, 1, eng.free_paths(only, **kw), 'dead outside the list')
    assert ((pair['ray_end'][1] == 0) & (pair['ray_segments'][1] > 0) & (pair['ray_segments'][1] < pair['ray_segments'][0])).sum() >= 100
    eng.close()


def test_partly_filled_workgroup():
    """'ttp' with a list of 201 entries (the 200 and one more mode: the last workgroup holds one wave) and n = 100 (a lane's second
    ray: the lane sums rest in device memory in between; the second pass of lanes is partly empty)."""
    ct, ref, kw = call_args('ttp')
    extra = np.setdiff1d(FC.active_modes(ct), ref['modes'])[:1]
    modes = np.concatenate([ref['modes'], extra]).astype(np.int32)
    assert modes.shape[0] == 201
    kw = dict(kw, modes=modes, x0=FC.uniform_points(ct, 201, kw['n'], 8))
    taus = columns(ct, modes)
    eng = fp_engine(ct, seed=4)
    cols = eng.free_path_columns(taus, **kw)
    for c in range(5):
        assert_column_is_single(cols, c, eng.free_paths(taus[c], **kw), '201 entries')
    # three rays per lane (n = 130) from the device sampler: the lane sums are read back and added to
    kw = dict(n=130, modes=modes[:7], max_segments=64, seed=17, rays=True)
    cols = eng.free_path_columns(taus, **kw)
    for c in range(5):
        assert_column_is_single(cols, c, eng.free_paths(taus[c], **kw), 'n = 130, device sampler')
    eng.close()


def test_list_longer_than_the_grid():
    """n > 64 and more than 4096 modes: the launch is capped at 1024 workgroups whose waves walk the list (the lane sums' scratch
    area is per wave of the grid), so a wave flies several modes one after another.  Every active mode of 'ttp' (4368), n = 70,
    16 segments, two columns against their single calls, rows and counts as bytes; a row does not depend on the grid."""
    ct = FC.case('ttp')
    act = FC.active_modes(ct)
    assert act.shape[0] > 4096
    taus = columns(ct, act)[[0, 3]]
    kw = dict(n=70, modes=act, max_segments=16, seed=29)
    eng = fp_engine(ct, seed=6)
    cols = eng.free_path_columns(taus, **kw)
    for c in range(2):
        one = eng.free_paths(taus[c], **kw)
        for k in SUMS:
            assert cols[k][c].tobytes() == one[k].tobytes(), (c, k)
        for k in COUNTS:
            assert int(cols[k][c]) == one['report'][k], (c, k)
    assert cols['capped'][1] > 0 and cols['report']['rays'] == act.shape[0] * 70
    # the same rows from a list short enough for one wave per mode: the last 100 modes
    tail = eng.free_path_columns(taus, **dict(kw, modes=act[-100:]))
    for k in SUMS:
        assert tail[k].tobytes() == cols[k][:, -100:].tobytes(), k
    eng.close()


@pytest.mark.parametrize('name', CASES)
def test_columns_do_not_see_each_other(name):
    """Column 1's rows (and rays) from the five-column call equal those from a two-column call {1, 3}; so do column 3's."""
    ct, taus, cols, singles = device_runs(name)
    _, ref, kw = call_args(name)
    eng = fp_engine(ct, seed=99)
    two = eng.free_path_columns(taus[[0, 2]], **kw)
    eng.close()
    for k in SUMS + RAYS:
        assert two[k][0].tobytes() == cols[k][0].tobytes() and two[k][1].tobytes() == cols[k][2].tobytes(), k
    for k in COUNTS:
        assert two[k][0] == cols[k][0] and two[k][1] == cols[k][2], k


@pytest.mark.parametrize('name', CASES)
def test_against_the_restatement(name):
    """Every column against free_path_cases.restate with that column's lifetimes, ray by ray: end codes and segment counts equal,
    displacements and flight times within test_gpu_free_path.py's bounds, the row sums the kernel's sum of its rays.  The facets a
    ray meets do not depend on the column (one flight): the restatement's sequence of a column is that of the first column wherever
    both made the same number of casts.  Rays whose facets hinge on the rounding of a hit point (free_path_cases.parity_run with
    the hit point as a product and a sum) are left out, as there.  The weights of a mode (each / n) are held to the bound of the
    reals, 5e-14, not to TOL_MODE_W: that one was measured on the first column, whose rays arrive at the cap with W ~ 1e-3; the
    fourth column's arrive with W ~ 1, a product of 256 factors e that each carry the roundings the flight times carry."""
    ct, taus, cols, singles = device_runs(name)
    p = FC.PARITY[name]
    ref0, other = FC.parity_run(name), FC.parity_run(name, fused=False)
    keep = ref0['ray_seq'] == other['ray_seq']
    assert 1.0 - keep.mean() <= FC.MAX_OTHER_SEQUENCE
    n = int(ref0['n'])
    for c in range(5):
        ref = ref0 if c == 0 else FC.cached(('free_sweep', 'restate', name, c), lambda: FC.restate(
            ct['mesh'], FC.group_vel(ct), taus[c], ref0['modes'], n, x0=ref0['ray_x0'], seed=p['seed'], max_segments=p['max_segments'],
            rough=ct['rough'], J=ct['J']))
        tag = '%s column %d' % (name, c)
        same = ref['ray_segments'] == ref0['ray_segments']
        assert np.array_equal(ref['ray_seq'][same], ref0['ray_seq'][same]), tag + ': the restatement flies another path'
        assert np.array_equal(cols['ray_end'][c][keep], ref['ray_end'][keep]), tag + ': end codes differ'
        assert np.array_equal(cols['ray_segments'][c][keep], ref['ray_segments'][keep]), tag + ': segment counts differ'
        nrm = np.linalg.norm(ref['ray_D'], axis=2)[..., None]
        nrm = np.where(nrm > 0, nrm, 1.0)
        assert allclose((cols['ray_D'][c] / nrm)[keep], (ref['ray_D'] / nrm)[keep], rtol=0, atol=TOL_RAY_D, tag=tag + ' D')
        assert rel_err(cols['ray_T'][c][keep], ref['ray_T'][keep], tag=tag + ' T', bound=TOL_RAY_T) <= TOL_RAY_T
        assert cols['D'][c].tobytes() == wave_sum(cols['ray_D'][c]).tobytes() and cols['T'][c].tobytes() == wave_sum(cols['ray_T'][c]).tobytes()
        assert rel_err(cols['D2'][c], wave_sum(cols['ray_D'][c] ** 2), tag=tag + ' D2', bound=n * 2.0 ** -53) <= n * 2.0 ** -53
        if keep.all():
            for k in ('p_res', 'p_wall', 'w_left', 'p_int'):
                assert allclose(cols[k][c] / n, ref[k] / n, rtol=0, atol=TOL_RAY_T, tag=tag + ' ' + k), k
            assert allclose(cols['hits'][c] / n, ref['hits'] / n, rtol=TOL_RAY_T, atol=TOL_MODE_W, tag=tag + ' hits')
            for k in COUNTS:
                assert int(cols[k][c]) == ref['report'][k], (tag, k)


def test_closed_form_and_invariant_per_column():
    """'ttp', every active mode, n = 64, start points drawn on the device, `scale` columns 0.5, 1, 2, 4 (lifetimes tau / s): the
    invariant p_res + p_wall + w_left + p_int = n per column to the bound of test_closed_form_and_invariant_on_device (1e-12);
    kappa_xx of column c, as the structure scaled by s_c, within 4 of ITS standard errors -- from the squares the call returns --
    of the closed form at L s_c."""
    from nanokappa_amd import free_path as FP, free_sweep as FS
    ct = FC.case('ttp')
    act = FC.active_modes(ct)
    tau = FC.lifetimes(ct)
    scales = np.array([0.5, 1.0, 2.0, 4.0])
    taus = FS.columns_scale(tau, scales)
    eng = fp_engine(ct, seed=1234)
    got = eng.free_path_columns(taus, n=64)
    one = eng.free_paths(tau, n=64)
    eng.close()
    assert np.array_equal(got['modes'], act) and np.all(got['missed'] == 0) and np.all(got['p_wall'] == 0)
    for k in SUMS:
        assert got[k][1].tobytes() == one[k].tobytes(), k                 # the device sampler's points are the single call's
    v = FC.group_vel(ct)[act]
    om = np.asarray(ct['tables']['omega'], dtype=float).ravel()[act]
    C = FP.mode_heat_capacity(om, FC.T_CASE, ct['tables']['hbar'], ct['tables']['kb'])
    for c, s in enumerate(scales):
        col = FS.scaled_column(FS.column(got, c), s)
        inv = invariant(col)
        assert allclose(inv, np.zeros_like(inv), rtol=0, atol=1e-12, tag='invariant, scale %g' % s)
        D, var = FP.mean_displacement(col)
        k, kse = FP.kappa_tensor(C, v, D, ct['tables']['QV'], var)
        cfD = np.zeros_like(D)
        cfD[:, 0] = FP.film_displacement(v[:, 0], tau[act], L_BOX * s)
        kcf = FP.kappa_tensor(C, v, cfD, ct['tables']['QV'])
        z = abs(k[0, 0] - kcf[0, 0]) / kse[0, 0]
        print('scale %g: kappa_xx %.6f +- %.6f W/m K, closed form at L = %g: %.6f (%.2f s.e.)' % (s, k[0, 0], kse[0, 0], L_BOX * s, kcf[0, 0], z))
        assert z <= 4.0
        assert np.all(D[v[:, 0] == 0, 0] == 0.0)
    print('device: %d casts for 4 columns (%d summed over the columns) in %.4f s' % (got['report']['casts_shared'], got['casts'].sum(), got['report']['seconds']))


def test_does_not_interfere_with_the_steps():
    """20 steps with a column call after step 10 against 20 steps without: the shape, and the tolerances for the four sums added
    with FP64 LDS atomics, of test_gpu_free_path.py's test."""
    from test_gpu_replicas import assert_same_rows, assert_same_particles
    ct = FC.case('ttp')
    pos, mode, occ, counter = random_population(ct, 30000, seed=5)
    modes = FC.spread_modes(ct, 40)
    taus = columns(ct, modes)
    engs, rows = [], []
    for with_call in (False, True):
        eng = make_engine(ct, pos, mode, occ, counter, seed=42)
        t0 = eng.step(10)
        if with_call:
            r = eng.free_path_columns(taus, n=64, modes=modes)
            assert r['report']['rays'] == 40 * 64 and r['report']['calls'] == 1 and eng.get_step() == 10
            assert eng.free_paths_info()['calls'] == 0
        t1 = eng.step(10)
        engs.append(eng)
        rows.append((t0, t1))
    assert_same_rows(rows[1][0], rows[0][0], 'steps 1-10')
    assert_same_rows(rows[1][1], rows[0][1], 'steps 11-20, after the call')
    assert_same_particles(engs[1], engs[0], 'after 20 steps')
    for e in engs:
        e.close()


def test_refusals():
    """K = 0, K = 33, a tau of the wrong shape, 'R' facets without tables, and nk_free_paths' own refusals in its words:
    NK_ERR_ARG with a text, and nothing launched (the next call is the engine's first)."""
    from nanokappa_amd.engine import Engine, NkError
    ct = FC.case('ttp')
    tau = FC.lifetimes(ct)
    M = ct['M']
    two = np.stack([tau, tau / 2.0])

    def refused(eng, text, **kw):
        args = dict(taus=two, n=8, modes=np.arange(4, dtype=np.int32))
        args.update(kw)
        with pytest.raises(NkError, match=r'\(-2\)') as e:
            eng.free_path_columns(args.pop('taus'), **args)
        assert text in str(e.value), str(e.value)

    eng = Engine(0, 1)
    refused(eng, 'no material')
    eng.set_material(ct['tables'])
    refused(eng, 'no mesh')
    eng.close()
    eng = fp_engine(ct)
    refused(eng, 'n_columns = 0', taus=np.zeros((0, M)))
    refused(eng, 'n_columns = 33', taus=np.stack([tau] * 33))
    refused(eng, 'taus must be', taus=tau)
    refused(eng, 'taus must be', taus=two[:, :-1])
    refused(eng, 'tau is NULL', taus=None)
    refused(eng, 'n_samples', n=0)
    refused(eng, 'out of range', modes=np.array([0, M], dtype=np.int32))
    r = eng.free_path_columns(two, n=8, modes=np.arange(4, dtype=np.int32))
    assert r['report']['calls'] == 1 and r['report']['rays'] == 32            # nothing ran before
    eng.close()
    eng = fp_engine(ct, volume=False)
    refused(eng, 'volume tables')
    eng.close()
    eng = fp_engine(FC.case('ttrrp'), rough=False)
    refused(eng, 'rough')
    eng.close()


def _ttp_argv(particles, iterations, extra=()):
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden'))
    import ref_harness_args as A
    return A.argv_for('ttp', particles, iterations) + ['--seed', '7'] + list(extra)


def test_front_end(tmp_path):
    """--free_path 16 --free_path_sweep scale 1 2 on the small box writes both sweep files; column `scale 1` reproduces
    k_free_path.txt's kappa, kappa_se and kappa_bulk digit for digit; with --free_path alone the sweep files are absent."""
    from nanokappa_amd import nanokappa, free_path as FP, free_sweep as FS

    def run(name, extra):
        pf = tmp_path / (name + '.txt')
        pf.write_text(' '.join(_ttp_argv(20000, 10, ['--results_folder', str(tmp_path / name)] + extra)))
        cwd = os.getcwd()
        os.chdir(str(tmp_path))
        try:
            return nanokappa.main(['-ff', str(pf)])
        finally:
            sys.stdout = sys.__stdout__
            os.chdir(cwd)

    pop = run('with', ['--free_path', '16', '--free_path_sweep', 'scale', '1', '2'])
    folder = pop.results_folder_name
    txt = FP.read_k_free_path(FP.k_free_path_path(folder))
    sw = FS.read_k_free_path_sweep(FS.k_free_path_sweep_path(folder))
    z = FS.read_free_path_sweep_npz(FS.free_path_sweep_npz_path(folder))
    assert sw['kind'] == 'scale' and sw['N'] == 16 and np.array_equal(sw['values'], [1.0, 2.0]) and z['kind'] == 'scale'
    for k in ('kappa', 'kappa_se', 'kappa_bulk'):
        assert sw[k][0] == txt[k][0, 0], k
        assert np.array_equal(z[k][0], txt[k]), k
    assert sw['kappa'][1] > sw['kappa'][0] and sw['kappa_bulk'][1] == sw['kappa_bulk'][0]
    assert pop.free_path_sweep_last['report']['calls'] == 1 and pop.free_path_report()['calls'] == 1 and pop.current_timestep == 10
    # Population.free_path_sweep with its own arguments: temperatures, no files
    t = pop.free_path_sweep('temperature', [250.0, 300.0], n=16, write=False)
    assert [c['T'] for c in t['columns']] == [250.0, 300.0] and np.allclose(t['columns'][1]['kappa'], pop.free_path_last['kappa'], rtol=1e-12, atol=0)
    pop.engine.close()

    pop = run('without', ['--free_path', '16'])
    folder = pop.results_folder_name
    assert os.path.exists(FP.k_free_path_path(folder))
    assert not os.path.exists(FS.k_free_path_sweep_path(folder)) and not os.path.exists(FS.free_path_sweep_npz_path(folder))
    pop.engine.close()
