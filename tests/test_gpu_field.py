"""Spatial field maps on the GPU (nk_set_field / k_field): state mode against the host restatement, step mode against the
step's own history row and against the oracle's particles, bit-identical runs and paths (LDS bins / global integer adds), the
field leaving every other output alone, the STL wire, the error paths, and the Population outputs (field.vtk)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from util import (case_tables, random_population, make_oracle_sim, make_engine, same_event_rule, rel_row, allclose,
                  assert_runs_equal, TOL_ROW_ERAW, TOL_ROW_FLUX, TOL_X, TOL_OCC)

pytestmark = pytest.mark.gpu

# State mode against the host: what the device's own e_i may cost on top of the rounding of the terms, relative to the largest
# cell.  Measured on an MI355X (profiles/r06_parity_margins.txt, `field state ... integers against the host integers`): 0 --
# the host forms e_i from the engine's own occupation tap (Engine.eval), and the device's integers then equal the host's
# integers of the host's terms bit for bit (two cases of 20 000 particles, E and the three components of F).  10 x 0 = 0: the
# integers must be equal.  The float64 sums are held to the derived bounds alone: n_cell 2^-(k+1) for the rounding of the
# terms plus n_cell 2^-53 max |term| for the host's own float additions.
# The equality rests on NumPy's hbar * omega * (n - n0) and v * e rounding exactly as the device's do -- true while the device
# expression holds no multiply-add the compiler may contract (one subtraction, then products).  A change of compiler or of the
# order of that expression would show here as a difference of one unit: then re-measure, do not widen blindly.
TOL_FIELD_STATE = 0.0


def grid_for(ct, per_slice=2, ny=4, nz=4):
    """(lo, h, n) over the case's bounding box, `per_slice` cells per slice subvolume along the slice axis."""
    from nanokappa_amd import field as FD
    S, a = ct['centers'].shape[0], ct['axis']
    n = [ny, nz, nz]
    n[a] = per_slice * S
    return FD.grid_from_bounds(ct['mesh']['bounds'], n)


def per_slice(a, axis, S):
    """Cells (nx, ny, nz[, 3]) summed per slice along `axis`: [S] or [S, 3]."""
    a = np.moveaxis(np.asarray(a), axis, 0)
    k = a.shape[0] // S
    a = a.reshape((S, k) + a.shape[1:])
    return a.sum(axis=(1, 2, 3))                       # (S, k, ., .[, 3]) -> (S[, 3])


def quant_bound(n, k):
    """Rounding of n terms to multiples of 2^-k: each within 2^-(k+1)."""
    return np.asarray(n, dtype=float) * np.ldexp(1.0, -(int(k) + 1))


def state_on_host(eng, ct):
    """Particles and their e_i the way state mode means them: occupations after the relaxation against the occupation at each
    particle's interpolated temperature (the expression of test_gpu_spectral.test_state_mode_against_host)."""
    p = eng.download()
    x, m, n = p['positions'], p['mode'].astype(int), p['occupation']
    T = eng.eval('interp_T', x)
    om = ct['ph'].omega.ravel()[m]
    n0 = np.where(T > 0, eng.eval('occupation', T, m), 0.0)
    e = ct['ph'].hbar * om * (n - n0)
    v = np.asarray(ct['tables']['group_vel']).reshape(-1, 3)[m]
    return x, e, v


def check_against_row(f, t, s, ct, info, label=''):
    """One sample's field against row s of the same step: the cells of a slice add up to the subvolume's tallies."""
    S, a = ct['centers'].shape[0], ct['axis']
    N = per_slice(f['N'], a, S)
    assert np.array_equal(N, t['N_sv'][s]), 'cells per slice against N_sv %s' % label
    E, F = per_slice(f['E'], a, S), per_slice(f['F'], a, S)
    dE = np.abs(E - t['E_raw'][s])
    bE = quant_bound(N, info['k_E']) + TOL_ROW_ERAW * np.max(np.abs(t['E_raw'][s]))
    assert np.all(dE <= bE), 'E against E_raw %s: %r over %r' % (label, dE.max(), bE.max())
    dF = np.abs(F - t['flux_raw'][s])
    bF = quant_bound(N, info['k_F'])[:, None] + TOL_ROW_FLUX * np.max(np.abs(t['flux_raw'][s]))
    assert np.all(dF <= bF), 'F against flux_raw %s: %r over %r' % (label, dF.max(), bF.max())
    rel_row(E, t['E_raw'][s], tag='field E per slice')
    rel_row(F, t['flux_raw'][s], tag='field F per slice')


# ---------------------------------------------------------------------------------------------- 1. state mode
@pytest.mark.parametrize('case', ['ttp', 'ttrrp'])
def test_state_mode_against_host(case):
    from nanokappa_amd import field as FD
    ct = case_tables(case)
    pos, mode, occ, counter = random_population(ct, 20000, seed=12, T0=303.0)     # 5 K above the subvolumes: e_i of full size
    eng = make_engine(ct, pos, mode, occ, counter, seed=2)
    lo, h, n = grid_for(ct)
    eng.set_field(lo, h, n, 10)
    eng.step(7)
    st = eng.tally_field_state()
    x, e, v = state_on_host(eng, ct)
    ref = FD.field_from_particles(x, e, v, lo, h, n)
    assert np.array_equal(st['N'], ref['N'])
    assert st['clamped'] == ref['clamped']
    assert st['N'].sum() == x.shape[0] == eng.timing()['live']
    assert not st['raw'][..., 5:].any()
    for key, k in (('E', st['k_E']), ('F', st['k_F'])):
        nb = ref['N'] if key == 'E' else ref['N'][..., None]
        term = np.max(np.abs(e)) if key == 'E' else np.max(np.abs(v * e[:, None]))
        dev = np.abs(st[key] - ref[key]) - quant_bound(nb, k) - nb * np.ldexp(term, -53)
        worst = float(np.max(dev) / np.max(np.abs(ref[key])))
        rel_row(st[key], ref[key], tag='field state ' + key)
        print('state mode %s: deviation less the rounding bound: %.3e of the largest cell' % (key, worst))
        assert worst <= TOL_FIELD_STATE
    # the integers against the host's own integers: the count plane is exact whatever the device's exp does, and pins the cell
    # indexing; the reals are the same integers wherever the host's term equals the device's bit for bit
    q = FD.quantised(x, e, v, lo, h, n, st['k_E'], st['k_F'])
    assert np.array_equal(st['raw'][..., 0], q['raw'][..., 0])
    ones = FD.quantised(x, np.ones_like(e), np.zeros_like(v), lo, h, n, 0, 0)
    assert np.array_equal(st['raw'][..., 0], ones['raw'][..., 1])
    # what the device's own e_i costs: its integers against the host's integers of the host's terms, as a fraction of the
    # largest cell (recorded: TOL_FIELD_STATE is set from it)
    for key, sl, k in (('E', slice(1, 2), st['k_E']), ('F', slice(2, 5), st['k_F'])):
        du = np.max(np.abs(st['raw'][..., sl] - q['raw'][..., sl]))
        term_dev = float(np.ldexp(float(du), -k) / np.max(np.abs(ref[key])))
        rel_row(np.ldexp(st['raw'][..., sl].astype(float), -k), np.ldexp(q['raw'][..., sl].astype(float), -k),
                tag='field state %s integers against the host integers' % key, bound=TOL_FIELD_STATE)
        print('state mode %s: device integers against host integers: %d units, %.3e of the largest cell' % (key, du, term_dev))
        assert term_dev <= TOL_FIELD_STATE


def test_state_mode_fixed_reference_temperature():
    """--reference_temp as a number: state mode takes n0 at T_ref for every particle (the other branch of k_field<true>), and
    the bound of the terms follows T_ref where it lies above the material's range."""
    from nanokappa_amd import field as FD
    ct = case_tables('ttp')
    pos, mode, occ, counter = random_population(ct, 20000, seed=13, T0=303.0)
    eng = make_engine(ct, pos, mode, occ, counter, seed=2)
    T_ref = 300.0
    eng.set_params(dt=1.0, particle_density=ct['particle_density'], T_ref=T_ref, flux_every=10, contains_every=100, track_ids=True)
    lo, h, n = grid_for(ct)
    eng.set_field(lo, h, n, 10)
    eng.step(7)
    st = eng.tally_field_state()
    p = eng.download()
    x, m = p['positions'], p['mode'].astype(int)
    n0 = eng.eval('occupation', np.full(m.shape[0], T_ref), m)
    e = ct['ph'].hbar * ct['ph'].omega.ravel()[m] * (p['occupation'] - n0)
    v = np.asarray(ct['tables']['group_vel']).reshape(-1, 3)[m]
    ref = FD.field_from_particles(x, e, v, lo, h, n)
    q = FD.quantised(x, e, v, lo, h, n, st['k_E'], st['k_F'])
    assert np.array_equal(st['N'], ref['N']) and st['clamped'] == ref['clamped']
    assert np.array_equal(st['raw'], q['raw'])                      # (TOL_FIELD_STATE = 0: the same integers)
    # ... and the sums are those of e against T_ref, not against the subvolumes' temperatures
    x2, e2, v2 = state_on_host(eng, ct)
    assert np.max(np.abs(FD.field_from_particles(x2, e2, v2, lo, h, n)['E'] - st['E'])) > 1e-3 * np.max(np.abs(st['E']))
    for key, k in (('E', st['k_E']), ('F', st['k_F'])):
        nb = ref['N'] if key == 'E' else ref['N'][..., None]
        term = np.max(np.abs(e)) if key == 'E' else np.max(np.abs(v * e[:, None]))
        assert np.all(np.abs(st[key] - ref[key]) <= quant_bound(nb, k) + nb * np.ldexp(term, -53))
    # a reference above the material's range raises the bound the scales are derived from
    B0 = eng.field_info()['B_E']
    eng.set_params(dt=1.0, particle_density=ct['particle_density'], T_ref=2000.0, flux_every=10, contains_every=100, track_ids=True)
    eng.tally_field_state()
    assert eng.field_info()['B_E'] > B0


def test_split_of_the_particles_does_not_change_the_integers():
    """The property the integers are there for: the sum of the grids of two parts of an ensemble IS the grid of the whole, bit
    for bit -- what an all-reduce over ranks relies on.  It holds for identical per-particle terms and equal scales: state mode
    on freshly uploaded particles (every engine sees the uploaded subvolume temperatures), the scales derived for one capacity
    (nk_field.capacity, above all three stores) so that k_E and k_F agree (asserted)."""
    ct = case_tables('ttp')
    pos, mode, occ, counter = random_population(ct, 30000, seed=31, T0=303.0)
    lo, h, n = grid_for(ct)
    cut = 11000                                                     # an uneven split
    parts = [(slice(0, cut), 0), (slice(cut, None), cut), (slice(None), 0)]
    out = []
    for sl, off in parts:
        eng = make_engine(ct, pos[sl], mode[sl], occ[sl], counter, seed=2, pid_offset=off)
        eng.set_field(lo, h, n, 10, capacity=1 << 20)              # (above all three stores: one k_E, one k_F)
        st = eng.tally_field_state()
        out.append((st, eng.field_info()))
    (a, ia), (b, ib), (c, ic) = out
    assert (ia['k_E'], ia['k_F']) == (ib['k_E'], ib['k_F']) == (ic['k_E'], ic['k_F']) and ia['capacity'] == ic['capacity'] == 1 << 20
    assert min(ia['capacity'], ib['capacity']) >= 1 << 20
    assert a['raw'][..., 0].sum() == cut and b['raw'][..., 0].sum() == 30000 - cut
    assert np.array_equal(a['raw'] + b['raw'], c['raw'])
    assert a['clamped'] + b['clamped'] == c['clamped']
    assert np.abs(c['raw'][..., 1]).max() > 0 and np.abs(c['raw'][..., 2:5]).max() > 0


# ---------------------------------------------------------------------------------------------- 2. step mode, the history row
@pytest.mark.parametrize('case', ['ttp', 'ttrrp'])
def test_step_mode_against_history_row(case):
    ct = case_tables(case)
    pos, mode, occ, counter = random_population(ct, 20000, seed=5)
    eng = make_engine(ct, pos, mode, occ, counter, seed=3)
    lo, h, n = grid_for(ct)
    eng.set_field(lo, h, n, 10)
    info = eng.field_info()
    assert info['on'] == 1 and info['ncells'] == n[0] * n[1] * n[2] and info['bytes'] > 0
    for call in range(3):
        t = eng.step(10)
        f = eng.field(reset=True)
        assert f['samples'] == 1
        check_against_row(f, t, 9, ct, eng.field_info(), label='(step %d)' % (10 * call + 9))
        assert f['N'].sum() == t['N_sv'][9].sum() == eng.timing()['live']
    # without a reset the samples add up
    t = eng.step(30)
    f = eng.field()
    assert f['samples'] == 3
    assert np.array_equal(per_slice(f['N'], ct['axis'], ct['centers'].shape[0]), t['N_sv'][[9, 19, 29]].sum(axis=0))
    # every = 20 on flux_every = 10: only every other heat-flux step is a field step
    eng.set_field(lo, h, n, 20)
    eng.step(40)
    assert eng.field()['samples'] == 2


# ---------------------------------------------------------------------------------------------- 3. the oracle's particles
@pytest.mark.parametrize('case', ['ttp', 'ttrrp'])
def test_step_mode_against_oracle(case):
    from nanokappa_amd import field as FD
    ct = case_tables(case)
    pos, mode, occ, counter = random_population(ct, 20000, seed=5)
    sim = make_oracle_sim(ct, pos, mode, occ, counter, seed=3)
    eng = make_engine(ct, pos, mode, occ, counter, seed=3)
    same_event_rule(eng, sim)
    lo, h, n = grid_for(ct)
    eng.set_field(lo, h, n, 10)
    vg = np.asarray(ct['tables']['group_vel']).reshape(-1, 3)
    for call in range(3):
        t = eng.step(10)
        f = eng.field(reset=True)
        info = eng.field_info()
        for _ in range(10):
            sim.run_timestep()
        P = sim.P
        k = P.N
        ref = FD.field_from_particles(P.pos[:k], P.energy[:k], vg[P.mode[:k].astype(int)], lo, h, n)
        assert f['samples'] == 1
        assert np.array_equal(f['N'], ref['N']), 'cell counts differ from the oracle at step %d' % (10 * call + 9)
        assert f['clamped'] == ref['clamped']
        dE = np.abs(f['E'] - ref['E']) - quant_bound(ref['N'], info['k_E'])
        dF = np.abs(f['F'] - ref['F']) - quant_bound(ref['N'], info['k_F'])[..., None]
        # (TOL_ROW_*: relative to the largest |value| of the subvolume row the cells add up to)
        assert np.max(dE) <= TOL_ROW_ERAW * np.max(np.abs(t['E_raw'][9]))
        assert np.max(dF) <= TOL_ROW_FLUX * np.max(np.abs(t['flux_raw'][9]))
        rel_row(f['E'], ref['E'], tag='field E against the oracle')
        rel_row(f['F'], ref['F'], tag='field F against the oracle')


# ---------------------------------------------------------------------------------------------- 4. determinism and paths
def _run_field(ct, pop4, n, flags=0, nsteps=20, seed=3):
    from nanokappa_amd import field as FD
    pos, mode, occ, counter = pop4
    eng = make_engine(ct, pos, mode, occ, counter, seed=seed)
    lo, h, n = FD.grid_from_bounds(ct['mesh']['bounds'], n)
    eng.set_field(lo, h, n, 10, flags=flags)
    t = eng.step(nsteps)
    f = eng.field()
    st = eng.tally_field_state()
    return t, f, st, eng.field_info()


def test_identical_bits_across_runs_and_paths():
    from nanokappa_amd.engine import FIELD_GLOBAL
    ct = case_tables('ttp')
    pop4 = random_population(ct, 20000, seed=21)
    S, a = ct['centers'].shape[0], ct['axis']
    n = [4, 4, 4]
    n[a] = 2 * S
    runs = [_run_field(ct, pop4, n), _run_field(ct, pop4, n), _run_field(ct, pop4, n, flags=FIELD_GLOBAL)]
    assert runs[0][3]['lds_path'] == 1 and runs[1][3]['lds_path'] == 1 and runs[2][3]['lds_path'] == 0
    for r in runs[1:]:
        assert r[1]['samples'] == runs[0][1]['samples'] == 2
        for k in ('N', 'E', 'F'):
            assert r[1][k].tobytes() == runs[0][1][k].tobytes(), k
        assert r[2]['raw'].tobytes() == runs[0][2]['raw'].tobytes()
        assert r[1]['clamped'] == runs[0][1]['clamped'] and r[2]['clamped'] == runs[0][2]['clamped']


def test_forced_global_path_by_environment(monkeypatch):
    ct = case_tables('ttp')
    pop4 = random_population(ct, 5000, seed=22)
    r0 = _run_field(ct, pop4, (8, 4, 4), nsteps=10)
    monkeypatch.setenv('NK_FIELD_PATH', 'global')
    r1 = _run_field(ct, pop4, (8, 4, 4), nsteps=10)
    assert r0[3]['lds_path'] == 1 and r1[3]['lds_path'] == 0
    assert r0[1]['E'].tobytes() == r1[1]['E'].tobytes() and r0[2]['raw'].tobytes() == r1[2]['raw'].tobytes()


def test_large_grid_global_path():
    """64^3 cells (16 MB of integers: the global path) on 3e5 particles, coarsened on the host to one cell per slice."""
    ct = case_tables('ttp')
    S, a = ct['centers'].shape[0], ct['axis']
    pos, mode, occ, counter = random_population(ct, 300000, seed=23)
    eng = make_engine(ct, pos, mode, occ, counter, seed=6)
    from nanokappa_amd import field as FD
    n = [64, 64, 64]
    n[a] = 60                                           # 3 cells per slice: aligned to the 20 slices
    lo, h, n = FD.grid_from_bounds(ct['mesh']['bounds'], n)
    eng.set_field(lo, h, n, 10)
    info = eng.field_info()
    assert info['lds_path'] == 0 and info['bytes'] >= n[0] * n[1] * n[2] * (64 + 40)
    t = eng.step(10)
    f = eng.field(reset=True)
    assert f['samples'] == 1
    check_against_row(f, t, 9, ct, eng.field_info(), label='(64^3)')
    assert f['N'].sum() == eng.timing()['live']


# ---------------------------------------------------------------------------------------------- 5. nothing else moves
@pytest.mark.parametrize('case,gen', [('ttp', 0), ('ttrrp', 0), ('ttp', 2)])
def test_field_leaves_everything_else(case, gen):
    ct = case_tables(case)
    pos, mode, occ, counter = random_population(ct, 20000, seed=8)
    runs = []
    for on in (False, True):
        eng = make_engine(ct, pos, mode, occ, counter, seed=4, gen=gen)
        if on:
            lo, h, n = grid_for(ct)
            eng.set_field(lo, h, n, 10)
        else:
            info = eng.field_info()
            assert info['on'] == 0 and info['bytes'] == 0 and info['ncells'] == 0
        t = eng.step(25)
        runs.append((t, eng.download()))
    (t0, p0), (t1, p1) = runs
    # (two runs of the engine sum their tally rows in different orders: counts and ids exactly, reals as assert_runs_equal
    # and the band pass's counterpart of this test hold two such runs)
    assert sorted(t0) == sorted(t1)
    assert_runs_equal(t0, t1)
    i0, i1 = np.argsort(p0['pid']), np.argsort(p1['pid'])
    assert np.array_equal(p0['pid'][i0], p1['pid'][i1])
    assert np.array_equal(p0['mode'][i0], p1['mode'][i1])
    assert allclose(p0['positions'][i0], p1['positions'][i1], rtol=0, atol=TOL_X)
    assert allclose(p0['occupation'][i0], p1['occupation'][i1], rtol=TOL_OCC, atol=0)


def test_field_off_again_frees_everything():
    ct = case_tables('ttp')
    pos, mode, occ, counter = random_population(ct, 5000, seed=8)
    eng = make_engine(ct, pos, mode, occ, counter, seed=4)
    lo, h, n = grid_for(ct)
    eng.set_field(lo, h, n, 10)
    assert eng.field_info()['bytes'] > 0
    eng.set_field(lo, h, (0, 0, 0), 10)
    assert eng.field_info()['bytes'] == 0 and eng.field_info()['on'] == 0
    from nanokappa_amd.engine import NkError
    with pytest.raises(NkError):
        eng.field()
    eng.step(10)


# ---------------------------------------------------------------------------------------------- 6. the STL wire
def test_field_sum_equals_flux_wire():
    """The 5000-face STL wire (split sweep, k_events, rough walls with migration): all cells together hold every live particle
    and the heat flux of all subvolumes."""
    import bench
    from nanokappa_amd import synthetic, field as FD
    from nanokappa_amd.phonon import Phonon
    from nanokappa_amd.population import Population
    args, geo = bench.wire_geometry(200000)
    ph = Phonon(args, 0, material=synthetic.make_material(9, 'Si', temperatures=np.arange(200.0, 401.0, 10.0)))
    pop = bench.quiet(Population, args, geo, ph)
    eng = pop.engine
    lo, h, n = FD.grid_from_bounds(geo.bounds, (16, 16, 32))
    eng.set_field(lo, h, n, 10)
    for call in range(2):
        halts0 = eng.timing()['halts']
        t = eng.step(10)
        f = eng.field(reset=True)
        info = eng.field_info()
        halted = eng.timing()['halts'] > halts0
        # a field step is a sample unless the engine says it halted in this call (migrants that waited in an inbox while the
        # store grew, as for band rows): no silent skips
        assert f['samples'] == 1 or (halted and f['samples'] == 0), (f['samples'], halted)
        if f['samples'] == 0:
            continue
        live = t['N_sv'][9].sum()
        assert f['N'].sum() == live
        F, F0 = f['F'].sum(axis=(0, 1, 2)), t['flux_raw'][9].sum(axis=0)
        bound = quant_bound(live, info['k_F']) + 1e-12 * np.max(np.abs(t['flux_raw'][9]))
        assert np.all(np.abs(F - F0) <= bound), (F, F0, bound)


# ---------------------------------------------------------------------------------------------- error paths
def test_error_paths():
    from nanokappa_amd.engine import Engine, NkError, FIELD_TEST_SMALL_BOUND
    ct = case_tables('ttp')
    pos, mode, occ, counter = random_population(ct, 5000, seed=8, T0=303.0)    # (5 K above the subvolumes: e_i of full size)
    eng = make_engine(ct, pos, mode, occ, counter, seed=4)                  # flux_every = 10
    lo, h, n = grid_for(ct)
    for every in (0, -10, 15, 5):
        with pytest.raises(NkError, match='multiple of flux_every'):
            eng.set_field(lo, h, n, every)
    with pytest.raises(NkError, match='cells'):
        eng.set_field(lo, h, (512, 512, 128), 10)                           # 2^25 cells
    with pytest.raises(NkError, match='positive'):
        eng.set_field(lo, (10.0, 0.0, 10.0), n, 10)
    assert eng.field_info()['on'] == 0
    bare = Engine(0, 1)
    with pytest.raises(NkError, match='material'):
        bare.set_field(lo, h, n, 10)
    # a bound 2^40 times too small: every ordinary term exceeds it -- an error that names the sum, never wrapped integers
    eng.set_field(lo, h, n, 10, flags=FIELD_TEST_SMALL_BOUND)
    with pytest.raises(NkError, match='field overflow.*B_E'):
        eng.tally_field_state()
    with pytest.raises(NkError, match='field overflow.*B_E'):
        eng.step(10)
    # ... and the engine is usable afterwards
    eng.set_field(lo, h, n, 10)
    eng.step(10)
    assert eng.field()['samples'] == 1


# ---------------------------------------------------------------------------------------------- communicator
def test_field_through_single_rank_communicator(monkeypatch):
    from nanokappa_amd.engine import comm_unique_id
    ct = case_tables('ttp')
    pos, mode, occ, counter = random_population(ct, 20000, seed=9)
    lo, h, n = grid_for(ct)
    ref = make_engine(ct, pos, mode, occ, counter, seed=1)
    ref.set_field(lo, h, n, 10)
    ref.step(20)
    f0, s0 = ref.field(), ref.tally_field_state()
    monkeypatch.setenv('NK_FORCE_COMM', '1')
    eng = make_engine(ct, pos, mode, occ, counter, seed=1)
    eng.comm_init(comm_unique_id(), 0, 1)
    eng.set_field(lo, h, n, 10)
    eng.step(20)
    f1, s1 = eng.field(), eng.tally_field_state()
    assert f0['samples'] == f1['samples'] == 2 and f0['clamped'] == f1['clamped']
    for k in ('N', 'E', 'F'):
        assert f0[k].tobytes() == f1[k].tobytes(), k
    assert s0['raw'].tobytes() == s1['raw'].tobytes()


# ---------------------------------------------------------------------------------------------- 7. Population
def test_population_end_to_end(tmp_path, capsys):
    """A parameter-file run with --field_grid 8 4 4 10 writes field.vtk beside the other outputs; the file holds what
    Population.field() returns; the accumulator restarts with the convergence window."""
    import bench
    from nanokappa_amd import nanokappa, field as FD
    argv, species, _ = bench.config_argv('c2', 100000, 200.0)
    argv = argv + ['--seed', '7', '--field_grid', '8', '4', '4', '10', '--iterations', '120', '--results_folder',
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
    path = FD.field_path(pop.results_folder_name)
    assert os.path.exists(path)
    r = FD.read_vtk(path)
    f = pop.field()
    assert r['n'] == (8, 4, 4) == f['n'] and np.array_equal(r['lo'], f['lo']) and np.array_equal(r['h'], f['h'])
    for k in ('N', 'T', 'energy', 'heat_flux'):
        assert np.array_equal(r[k], f[k], equal_nan=True), k
    # n_mean = 5 rows of 10 steps, every = 10: windows of 50 steps.  After 120 steps the latest complete window is steps
    # 51..100: exactly its five field steps, whatever came after
    assert pop.field_window == 50 and f['samples'] == 5
    assert pop.engine.field()['samples'] == 2                   # (steps 110 and 120 of the window in progress)
    assert np.all(f['N'] > 0) and np.all(np.isfinite(f['T'])) and np.all(np.isfinite(f['heat_flux']))
    # mean particles per field step over the cells = the ensemble; the temperatures lie between the reservoirs'
    assert abs(f['N'].sum() - pop.N_p) <= 0.02 * pop.N_p
    lo_T, hi_T = float(np.min(pop.res_facet_temperature)), float(np.max(pop.res_facet_temperature))
    assert np.all(f['T'] > lo_T - 5.0) and np.all(f['T'] < hi_T + 5.0)
    from nanokappa_amd.field import field_grid_option
    assert field_grid_option(getattr(pop.args, 'field_grid', None))[0] == (8, 4, 4)
    # another grid: nothing of the old one is left behind
    pop.set_field((4, 4, 2), 20)
    assert pop.field()['samples'] == 0 and pop.field()['N'].shape == (4, 4, 2)
    pop.run(80)                                                 # to step 200: windows of 40 steps (5 rows = 50 steps, two field steps)
    g = pop.field()
    assert pop.field_window == 40 and g['samples'] == 2 and g['N'].shape == (4, 4, 2)


def _field_pop(extra=()):
    import bench
    from nanokappa_amd import synthetic
    from nanokappa_amd.argument_parser import initialise_parser
    from nanokappa_amd.geometry import Geometry
    from nanokappa_amd.phonon import Phonon
    from nanokappa_amd.population import Population
    argv, species, _ = bench.config_argv('c2', 50000, 200.0)
    args = initialise_parser().parse_args(argv + ['--seed', '11', '--n_mean', '3', '--field_grid', '8', '4', '4', '10'] + list(extra))
    args.results_folder = ''
    geo = bench.quiet(Geometry, args)
    ph = Phonon(args, 0, material=synthetic.make_material(31, species, temperatures=np.arange(200.0, 401.0, 10.0)))
    return bench.quiet(Population, args, geo, ph)


def test_window_does_not_depend_on_how_the_run_is_cut():
    """run(70) in one go, step by step, and in uneven pieces: the same windows (30 steps: 3 rows), the same sample counts, the
    same particle counts per cell; the reals as two runs of the engine agree (their tallies are summed in different orders)."""
    from util import TOL_RUN_ERAW, TOL_T
    fields = []
    for pieces in ([70], [1] * 70, [7, 13, 29, 21]):
        pop = _field_pop()
        assert pop.field_window == 30
        for k in pieces:
            bench_quiet_run(pop, k)
        fields.append((pop.field(), pop.engine.field()))
    (f0, r0) = fields[0]
    assert f0['samples'] == 3 and r0['samples'] == 1            # window 31..60 complete; step 70 in progress
    for f, r in fields[1:]:
        assert f['samples'] == f0['samples'] and r['samples'] == r0['samples']
        assert np.array_equal(f['N'], f0['N']) and np.array_equal(r['N'], r0['N'])
        assert np.max(np.abs(f['energy'] - f0['energy'])) <= TOL_RUN_ERAW * np.max(np.abs(f0['energy']))
        # (a term is C_i (T_i - T_sv) with differences of the order of 1 K, and two runs' T_sv agree to TOL_T kelvin: 2e-11 of it)
        assert np.max(np.abs(f['heat_flux'] - f0['heat_flux'])) <= TOL_T * np.max(np.abs(f0['heat_flux']))


def bench_quiet_run(pop, k):
    import bench
    bench.quiet(pop.run, k)


def test_fig_plot_points_to_field_grid(tmp_path, capsys):
    import bench
    from nanokappa_amd.argument_parser import initialise_parser
    from nanokappa_amd.geometry import Geometry
    from nanokappa_amd.phonon import Phonon
    from nanokappa_amd.population import Population
    from nanokappa_amd import synthetic
    argv, species, _ = bench.config_argv('c2', 20000, 200.0)
    args = initialise_parser().parse_args(argv + ['--seed', '3', '--fig_plot', 'T', 'e'])
    args.results_folder = ''
    geo = bench.quiet(Geometry, args)
    ph = Phonon(args, 0, material=synthetic.make_material(31, species, temperatures=np.arange(200.0, 401.0, 10.0)))
    pop = Population(args, geo, ph)
    out = capsys.readouterr().out
    assert out.count('--field_grid') == 1 and pop.field_n is None
    assert pop.engine.field_info()['bytes'] == 0
