"""Free-path sampling on the GPU (Engine.free_paths; k_free_paths) against its CPU restatement (tests/free_path_cases.py), ray
by ray with the start points given; the device sampler; the closed form and the invariant; determinism; non-interference with
the steps; the refusals; Population.free_paths and --free_path.

Tolerances of the per-ray comparisons: <= 10 x the largest deviation measured on an MI355X (profiles/free_path_margins.txt;
recorded by tests/util.py at every call site), the project's rule.  Displacements are compared relative to the ray's own |D|
(its components can cancel after a specular reflection), flight times relative to themselves."""
import os
import sys

import numpy as np
import pytest

import free_path_cases as FC
from util import allclose, rel_err, make_engine, random_population
from test_free_path_host import closed_form_checks, invariant

pytestmark = pytest.mark.gpu

# Per ray, kernel against restatement: each segment adds W tau g v with a handful of roundings (the division tc / tau, the series
# or exponential against NumPy's expm1 / exp, the products) and W carries the roundings of all segments before it.
# Measured on an MI355X (profiles/free_path_margins.txt): D 7.1e-15 and T 9.6e-15 on 'ttp' (up to 256 segments), the other
# cases 5.5e-16 .. 1.1e-15.
TOL_RAY_D = 5e-14          # max |D_gpu - D_cpu| / |D_cpu|_2 of a ray
TOL_RAY_T = 5e-14          # relative, flight time of a ray
# The weights of a mode (p_res, p_wall, w_left, p_int; each / n, so <= 1): measured <= 6.7e-16
TOL_MODE_W = 5e-15
# start points of the device sampler: four logarithms and a convex combination of a simplex's corners, coordinates up to 200
# angstrom (measured 5.7e-14 angstrom in the box, 1.1e-13 in the corrugated wire)
TOL_X0 = 8e-13


def wave_sum(a):
    """The kernel's sum of a mode's rays, in its order: lane l adds samples l, l + 64, ... in ascending order, then the 64 lane
    sums are combined by a butterfly (xor 32, 16, .., 1).  a [L, n, ...] -> [L, ...], the same bits as the device's."""
    a = np.asarray(a, dtype=np.float64)
    L, n = a.shape[:2]
    lanes = np.zeros((L, 64) + a.shape[2:])
    for s0 in range(0, n, 64):
        m = min(64, n - s0)
        lanes[:, :m] = lanes[:, :m] + a[:, s0:s0 + m]
    idx = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        lanes = lanes + lanes[:, idx ^ o]
    return lanes[:, 0]


def fp_engine(ct, seed=5, rough=True, volume=True):
    """An engine with the tables of a case and NO particles."""
    from nanokappa_amd.engine import Engine
    eng = Engine(0, seed)
    eng.set_material(ct['tables'])
    g = ct['mesh']
    if not volume:
        g = {k: v for k, v in g.items() if not k.startswith('simplices')}
    eng.set_mesh(g)
    S = ct['centers'].shape[0]
    eng.set_subvolumes(ct['centers'], ct['volumes'], ct.get('kind', 0), ct['axis'], 1 if ct.get('kind', 0) == 0 else 2, np.full(S, 300.0))
    if rough and ct['rough'] is not None:
        r = ct['rough']
        eng.set_rough(r['facets'], r['specularity'], r['true_spec'], r['spec_map'], r['roulette'], degen_j2=r.get('degen_j2'))
    return eng


def run_parity(name):
    p = FC.PARITY[name]
    ct = FC.case(p['case'])
    ref = FC.parity_run(name)
    other = FC.parity_run(name, fused=False)
    eng = fp_engine(ct, seed=99)                       # (the call's seed is given: the engine's must not matter)
    got = eng.free_paths(FC.lifetimes(ct), n=p['n'], modes=ref['modes'], max_segments=p['max_segments'], x0=ref['ray_x0'],
                         seed=p['seed'], rays=True)
    eng.close()
    return ct, ref, other, got


def assert_rays(name, ref, other, got):
    keep = ref['ray_seq'] == other['ray_seq']          # rays whose facets hinge on the rounding of a hit point are left out
    left_out = 1.0 - keep.mean()
    print('%s: %d rays, %.4f %% left out' % (name, keep.size, 100 * left_out))
    assert left_out <= FC.MAX_OTHER_SEQUENCE
    assert np.array_equal(got['ray_x0'], ref['ray_x0'])
    assert np.array_equal(got['ray_end'][keep], ref['ray_end'][keep]), 'end codes differ'
    assert np.array_equal(got['ray_segments'][keep], ref['ray_segments'][keep]), 'segment counts differ'
    nrm = np.linalg.norm(ref['ray_D'], axis=2)[..., None]
    nrm = np.where(nrm > 0, nrm, 1.0)
    assert allclose((got['ray_D'] / nrm)[keep], (ref['ray_D'] / nrm)[keep], rtol=0, atol=TOL_RAY_D, tag=name + ' D'), 'displacements differ'
    assert rel_err(got['ray_T'][keep], ref['ray_T'][keep], tag=name + ' T', bound=TOL_RAY_T) <= TOL_RAY_T, 'flight times differ'
    # a mode's row is the sum of its rays in the kernel's order: the same bits for D and T (plain adds); for the squares, which
    # the device may add with fused multiply-adds, one rounding per add: (n / 64 + 7) 2^-53 of a sum of positive terms
    n = int(ref['n'])
    assert got['D'].tobytes() == wave_sum(got['ray_D']).tobytes() and got['T'].tobytes() == wave_sum(got['ray_T']).tobytes()
    assert rel_err(got['D2'], wave_sum(got['ray_D'] ** 2), tag=name + ' D2', bound=n * 2.0 ** -53) <= n * 2.0 ** -53
    if keep.all():                                       # the other sums against the restatement's
        for k in ('p_res', 'p_wall', 'w_left', 'p_int'):
            assert allclose(got[k] / n, ref[k] / n, rtol=0, atol=TOL_MODE_W, tag=name + ' ' + k), k
        # hits = sum over the hits of W: the relative error of the flight times (sums of the same W, times tau g)
        assert allclose(got['hits'] / n, ref['hits'] / n, rtol=TOL_RAY_T, atol=TOL_MODE_W, tag=name + ' hits')
        for k in ('rays', 'casts', 'missed', 'capped'):
            assert got['report'][k] == ref['report'][k], k


def test_rays_ttp_with_cap_and_partial_pass():
    """200 modes of the T T P box including every fourth v_x = 0 mode, n = 100 (the second pass of lanes is partly empty),
    max_segments = 256 (the cap path runs)."""
    ct, ref, other, got = run_parity('ttp')
    assert got['report']['geometry_mode'] == 1 and got['report']['capped'] > 1000 and (got['ray_end'] == 4).any()
    assert (FC.group_vel(ct)[ref['modes'], 0] == 0).sum() >= 50
    assert_rays('ttp', ref, other, got)


@pytest.mark.parametrize('name', ['ttrrp', 'ttrrp_k'])
def test_rays_rough_box(name):
    """T T R R P with the 'velocity' tables and with the 'k' tables and degen_j2: specular continuation into another mode, and
    the diffuse end."""
    ct, ref, other, got = run_parity(name)
    assert (got['ray_end'] == 2).any() and (got['ray_end'] == 1).any()
    assert_rays(name, ref, other, got)


def test_rays_corrugated():
    """The non-convex corrugated wire: planes in LDS, the general search (a ray's nearest plane need not hold its hit)."""
    ct, ref, other, got = run_parity('corrugated')
    assert got['report']['geometry_mode'] == 1
    assert_rays('corrugated', ref, other, got)


def test_rays_wire72_tree():
    """The 72-sided cylinder: 288 faces, tables in global memory, the face tree."""
    ct, ref, other, got = run_parity('wire72')
    assert ct['mesh']['face_normals'].shape[0] > 256 and got['report']['geometry_mode'] == 2
    assert_rays('wire72', ref, other, got)


@pytest.mark.parametrize('name', ['ttp', 'corrugated'])
def test_device_sampler(name):
    """The start points the kernel draws are the restatement's draws, and lie inside the solid."""
    ct = FC.case(name)
    modes = FC.spread_modes(ct, 12)
    eng = fp_engine(ct, seed=31)
    got = eng.free_paths(FC.lifetimes(ct), n=70, modes=modes, rays=True)           # seed 0: the engine's
    eng.close()
    ref = FC.start_points(ct['mesh'], modes, 70, 31)
    assert allclose(got['ray_x0'], ref, rtol=0, atol=TOL_X0, tag=name)
    pts = got['ray_x0'].reshape(-1, 3)
    if name == 'ttp':
        b = np.asarray(ct['mesh']['bounds'], dtype=float)
        assert np.all(pts > b[0]) and np.all(pts < b[1])
    else:
        assert np.all(ct['geo'].mesh.contains(pts))
    assert np.unique(pts[:, 0]).size == pts.shape[0]                             # every ray its own draw
    assert got['report']['missed'] == 0


def test_closed_form_and_invariant_on_device():
    """'ttp', every active mode, n = 64, start points drawn on the device: the bounds of the CPU test (6 standard errors per
    mode, exactly 0 for v_x = 0, kappa_xx within 4).  The invariant p_res + p_wall + w_left + p_int = n in the same run: per
    segment g + e = 1 holds to 2 ulp (the series and nk_exp_small, or 1 - e exactly), weighted by the ray's W <= 1; a ray has at
    most ~1.1e4 segments here (W < 2^-40 ends it) but W decays geometrically, so the defect of a ray is a few ulp times the
    segments over which W is of order one (<= Lambda / L ~ 400): <= 400 x 2 x 1.1e-16 ~ 1e-13 per ray, and the same relative to n
    for a mode.  Bound 1e-12, as on the CPU."""
    ct = FC.case('ttp')
    act = FC.active_modes(ct)
    eng = fp_engine(ct, seed=1234)
    got = eng.free_paths(FC.lifetimes(ct), n=64)                                  # the default list
    assert np.array_equal(got['modes'], act) and got['report']['missed'] == 0 and got['report']['capped'] == 0
    closed_form_checks(ct, got, 'device')
    inv = invariant(got)
    assert allclose(inv, np.zeros_like(inv), rtol=0, atol=1e-12, tag='invariant')
    assert np.all(got['p_wall'] == 0) and got['report']['rays'] == act.size * 64
    print('device: %d casts in %.4f s' % (got['report']['casts'], got['report']['seconds']))
    assert eng.free_paths_info() == got['report']
    eng.close()


def test_determinism():
    """Two calls give the same bits; the rows of a 50-mode list equal those rows of the all-modes call bit for bit; another
    seed differs."""
    ct = FC.case('ttrrp')
    tau = FC.lifetimes(ct)
    act = FC.active_modes(ct)
    eng = fp_engine(ct, seed=77)
    keys = ('D', 'D2', 'T', 'hits', 'p_res', 'p_wall', 'w_left', 'p_int')
    a = eng.free_paths(tau, n=70)
    b = eng.free_paths(tau, n=70)
    for k in keys:
        assert a[k].tobytes() == b[k].tobytes(), k
    pick = np.sort(np.random.default_rng(3).choice(act.size, 50, replace=False))
    c = eng.free_paths(tau, n=70, modes=act[pick][::-1].copy())                   # (and in another order)
    for k in keys:
        assert c[k][::-1].tobytes() == a[k][pick].tobytes(), k
    d = eng.free_paths(tau, n=70, seed=78)
    assert d['D'].tobytes() != a['D'].tobytes() and not np.array_equal(d['p_res'], a['p_res'])
    e = eng.free_paths(tau, n=70, seed=77)                                        # the engine's seed, spelled out
    assert e['D'].tobytes() == a['D'].tobytes()
    eng.close()


def test_does_not_interfere_with_the_steps():
    """20 steps with a free_paths call after step 10 against 20 steps without: the same particles, counts, T_sv and E_sv bit for
    bit.  The four sums a workgroup's waves add with FP64 LDS atomics (E_raw, flux_raw, res_energy, res_flux) differ in their last
    bit between ANY two runs of this engine (tests/test_gpu_replicas.py, module docstring): they are held to the project's
    tolerance for two runs that sum in different orders, exactly as a group member is held against its solo run there."""
    from test_gpu_replicas import assert_same_rows, assert_same_particles
    ct = FC.case('ttp')
    pos, mode, occ, counter = random_population(ct, 30000, seed=5)
    tau = FC.lifetimes(ct)
    engs, rows = [], []
    for with_call in (False, True):
        eng = make_engine(ct, pos, mode, occ, counter, seed=42)
        t0 = eng.step(10)
        if with_call:
            r = eng.free_paths(tau, n=64, modes=FC.spread_modes(ct, 40))
            assert r['report']['rays'] == 40 * 64 and eng.get_step() == 10
        t1 = eng.step(10)
        engs.append(eng)
        rows.append((t0, t1))
    assert_same_rows(rows[1][0], rows[0][0], 'steps 1-10')
    assert_same_rows(rows[1][1], rows[0][1], 'steps 11-20, after the call')
    assert_same_particles(engs[1], engs[0], 'after 20 steps')
    for e in engs:
        e.close()


def test_refusals():
    """Every NK_ERR_ARG case, with a text that names the cause."""
    from nanokappa_amd.engine import Engine, NkError
    ct = FC.case('ttp')
    tau = FC.lifetimes(ct)
    M = ct['M']

    def refused(eng, text, **kw):
        args = dict(tau=tau, n=8, modes=np.arange(4, dtype=np.int32))
        args.update(kw)
        with pytest.raises(NkError, match=r'\(-2\)') as e:
            eng.free_paths(args.pop('tau'), **args)
        assert text in str(e.value), str(e.value)

    eng = Engine(0, 1)
    refused(eng, 'no material')
    eng.set_material(ct['tables'])
    refused(eng, 'no mesh')
    eng.close()
    eng = fp_engine(ct)
    refused(eng, 'n_samples', n=0)
    refused(eng, 'n_samples', n=-3)
    refused(eng, 'out of range', modes=np.array([0, M], dtype=np.int32))
    refused(eng, 'out of range', modes=np.array([-1], dtype=np.int32))
    refused(eng, 'tau is NULL', tau=None)
    assert eng.free_paths_info()['calls'] == 0                  # nothing ran
    eng.free_paths(tau, n=8, modes=np.arange(4, dtype=np.int32))
    eng.close()
    eng = fp_engine(ct, volume=False)
    refused(eng, 'volume tables')
    x0 = FC.uniform_points(ct, 4, 8, 1)
    assert eng.free_paths(tau, n=8, modes=np.arange(4, dtype=np.int32), x0=x0)['report']['rays'] == 32     # with x0 it runs
    eng.close()
    cr = FC.case('ttrrp')
    eng = fp_engine(cr, rough=False)
    refused(eng, 'rough')
    eng.close()


def _ttp_argv(particles, iterations, extra=()):
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden'))
    import ref_harness_args as A
    return A.argv_for('ttp', particles, iterations) + ['--seed', '7'] + list(extra)


def test_population_and_front_end(tmp_path):
    """--free_path 64 on 'ttp' writes k_free_path.txt and free_path.npz before the first step, with the numbers of the engine
    call; Population.free_paths returns them; without the option no file is written and the report says nothing was allocated."""
    from nanokappa_amd import nanokappa, free_path as FP

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

    pop = run('with', ['--free_path', '64'])
    folder = pop.results_folder_name
    assert os.path.exists(FP.k_free_path_path(folder)) and os.path.exists(FP.free_path_npz_path(folder))
    s = pop.free_path_last
    assert s['T'] == 300.0 and s['n'] == 64 and s['axis'] == 0 and pop.free_path_report()['calls'] == 1      # mean of 302 and 298 K
    ph = pop._ph
    tau = FP.lifetimes(ph, 300.0)
    eng_res = pop.engine.free_paths(tau, n=64)                     # the same call again: same seed, same bits
    for k, v in s['sums'].items():
        assert np.array_equal(v, eng_res[k]), k
    again = FP.summarise(eng_res, ph.omega, ph.group_vel, tau, ph.number_of_qpoints * ph.volume_unitcell, 300.0, axis=0, hbar=pop.hbar, kb=pop.kb)
    txt, z = FP.read_k_free_path(FP.k_free_path_path(folder)), FP.read_free_path_npz(FP.free_path_npz_path(folder))
    for k in ('kappa', 'kappa_se', 'kappa_bulk'):
        assert np.array_equal(txt[k], again[k]) and np.array_equal(z[k], again[k]), k
    assert np.array_equal(txt['grid'], again['accumulation']['grid']) and np.array_equal(txt['sampled'], again['accumulation']['sampled'])
    assert np.array_equal(txt['bulk'], again['accumulation']['bulk']) and txt['N'] == 64 and txt['missed'] == 0 and txt['capped'] == 0
    assert np.array_equal(z['modes'], eng_res['modes']) and np.array_equal(z['sum_D'], eng_res['D'])
    # the estimate itself: the closed form's 2.7 % of the bulk value along x, isotropic bulk
    assert 0.02 < again['kappa'][0, 0] / again['kappa_bulk'][0, 0] < 0.035
    # Population.free_paths with its own arguments: another temperature, a mode list, no files
    t = pop.free_paths(n=16, T=250.0, modes=eng_res['modes'][:30], write=False)
    assert t['T'] == 250.0 and t['sums']['D'].shape == (30, 3) and pop.free_path_report()['calls'] == 3
    assert pop.current_timestep == 10
    pop.engine.close()

    pop = run('without', [])
    folder = pop.results_folder_name
    assert not os.path.exists(FP.k_free_path_path(folder)) and not os.path.exists(FP.free_path_npz_path(folder))
    rep = pop.free_path_report()
    assert rep['calls'] == 0 and rep['bytes'] == 0 and rep['rays'] == 0
    pop.engine.close()
