"""Mode-resolved tally on the GPU (nk_set_modes / k_modes): step mode against the oracle's particles and against the step's own
history row, against the band pass, state mode against the host's integers and against the reference's own k(omega), the two
paths (owner / global) and splits of the ensemble bit for bit, a store that regrows in mid-window, the tally leaving every
other output alone, the error paths, a single-rank communicator."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from util import (case_tables, random_population, make_oracle_sim, make_engine, same_event_rule, rel_row, allclose,
                  assert_runs_equal, TOL_X, TOL_OCC)

pytestmark = pytest.mark.gpu

# Step mode against the ORACLE's particles, per (subvolume, mode) bin.  Two parts.  Derived: the rounding of the integers,
# n_bin 2^-(k_E + 1) (quant_bound).  Measured: what the engine's own e_i differ by from the oracle's on top of that (its
# occupations and subvolume temperatures agree with the oracle's to TOL_OCC / TOL_T, not bit for bit), as the largest excess
# of |E - E_oracle| over the rounding bound, relative to the largest |bin| of the oracle's table: 2.7e-14 at the worst on an
# MI355X over ttp, ttrrp and ttp under NK_NO_BOX, three mode steps each (2.2e-15 on the regrown stores).  The bound is 10 x
# that.  (The whole deviation, rounding included, is recorded in profiles/r07_parity_margins.txt, `modes E against the
# oracle`: 1.1e-11 of the largest bin.)
TOL_MODES_ORACLE = 2.7e-13
# Sums over the modes against the history row of the same step (E_raw, flux_raw) and against the band pass: the same terms
# e_i, added in two orders.  Derived: the rounding of the integers, n 2^-(k_E + 1) (times the largest |v| component for v E),
# plus the float64 additions and products of either side, n 2^-52 max |term| (float_bound).  Measured: the excess over the
# rounding bound alone -- none anywhere (the worst case is -9.9e-11 of the row's largest value, i.e. inside the bound, on the
# small cases, -7.1e-09 on config 2 at 1e7 particles, -5.6e-10 on the STL wire, 0 against the band pass): the roundings of n
# terms add up like sqrt(n), the bound takes n.  10 x 0 = 0: nothing is allowed beyond the two derived parts.
TOL_MODES_ROW = 0.0
# State mode: the device's integers against modes.quantised of the host's terms (formed from the engine's own taps): measured
# 0 units in all three cases, as test_gpu_field.py::test_state_mode_against_host establishes for the field; 10 x 0 = 0.
# Against the reference's own flux_contribution (tests/golden/k_contribution.npz): measured 1.3e-12 of max |k| (the band
# pass, which adds float64 terms, measured 1.5e-14 there; here every e_i is rounded to a multiple of 2^-k_E, 2^-52 eV on this
# small store against terms of 1e-5 eV); 10 x.
TOL_MODES_K_GOLDEN = 1.3e-11


def quant_bound(n, k):
    """Rounding of n terms to multiples of 2^-k: each within 2^-(k+1)."""
    return np.asarray(n, dtype=float) * np.ldexp(1.0, -(int(k) + 1))


def float_bound(n, term):
    """float64 sums of n terms of size <= term in two orders, each term a product rounded once: n 2^-52 term."""
    return np.asarray(n, dtype=float) * np.ldexp(float(term), -52)


def excess(a, b, qb):
    """What |a - b| exceeds the rounding bound qb by at the worst, relative to the largest |b| (negative: inside the bound).
    (The rel_row calls beside it record the WHOLE deviation, rounding included, for profiles/*parity_margins.txt; the
    tolerances apply to this excess.)"""
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b)) - qb) / max(np.max(np.abs(b)), 1e-300))


def vg_of(ct):
    return np.asarray(ct['tables']['group_vel']).reshape(-1, 3)


def check_against_row(m, t, s, ct, info, label=''):
    """One sample's table [S, Q, J] against row s of the same step's history."""
    from nanokappa_amd import modes as MD
    S = ct['centers'].shape[0]
    N, E = m['N'].reshape(S, -1), m['E'].reshape(S, -1)
    assert np.array_equal(N.sum(axis=1), t['N_sv'][s]), 'sum over the modes of N against N_sv %s' % label
    nsv = t['N_sv'][s]
    Es = E.sum(axis=1)
    dE = rel_row(Es, t['E_raw'][s], tag='modes sum E against E_raw')
    xE = excess(Es, t['E_raw'][s], quant_bound(nsv, info['k_E']) + float_bound(nsv, info['B_E']))
    print('modes against the row %s: sum E against E_raw %.3e of the largest, %.3e beyond the rounding bound' % (label, dE, xE))
    assert xE <= TOL_MODES_ROW, 'E against E_raw %s: %r' % (label, xE)
    Fs = MD.mode_flux(E, vg_of(ct)).sum(axis=1)
    dF = rel_row(Fs, t['flux_raw'][s], tag='modes sum v E against flux_raw')
    vmax = np.max(np.abs(vg_of(ct)))
    xF = excess(Fs, t['flux_raw'][s], vmax * (quant_bound(nsv, info['k_E']) + float_bound(nsv, info['B_E']))[:, None])
    print('modes against the row %s: sum v E against flux_raw %.3e of the largest, %.3e beyond the rounding bound' % (label, dF, xF))
    assert xF <= TOL_MODES_ROW, 'v E against flux_raw %s: %r' % (label, xF)


# ---------------------------------------------------------------------------------------------- 7. + 8. the oracle's particles
@pytest.mark.parametrize('case,nobox', [('ttp', False), ('ttrrp', False), ('ttp', True)])
def test_step_mode_against_oracle(case, nobox, monkeypatch):
    from nanokappa_amd import modes as MD
    if nobox:
        monkeypatch.setenv('NK_NO_BOX', '1')
    ct = case_tables(case)
    S, M = ct['centers'].shape[0], ct['M']
    pos, mode, occ, counter = random_population(ct, 20000, seed=5)
    sim = make_oracle_sim(ct, pos, mode, occ, counter, seed=3)
    eng = make_engine(ct, pos, mode, occ, counter, seed=3)
    same_event_rule(eng, sim)
    eng.set_modes(10)
    info = eng.modes_info()
    assert info['on'] == 1 and info['owner_path'] == 1 and info['bytes'] >= S * M * 28 and info['every'] == 10
    for call in range(3):
        t = eng.step(10)
        m = eng.modes(reset=True)
        info = eng.modes_info()
        for _ in range(10):
            sim.run_timestep()
        P = sim.P
        k = P.N
        ref = MD.table_from_particles(P.sv[:k].astype(int), P.mode[:k].astype(int), P.energy[:k], S, M)
        assert m['samples'] == 1 and m['skipped'] == 0
        N, E = m['N'].reshape(S, M), m['E'].reshape(S, M)
        assert np.array_equal(N, ref['N']), 'bin counts differ from the oracle at step %d' % (10 * call + 9)
        assert N.sum() == k
        d = rel_row(E, ref['E'], tag='modes E against the oracle')
        x = excess(E, ref['E'], quant_bound(ref['N'], info['k_E']))
        print('modes against the oracle, %s step %d: largest deviation %.3e of the largest bin, %.3e beyond the rounding bound'
              % (case, 10 * call + 9, d, x))
        assert x <= TOL_MODES_ORACLE
        check_against_row(m, t, 9, ct, info, label='(%s step %d)' % (case, 10 * call + 9))
    # without a reset the samples add up; every = 20 on flux_every = 10: every other heat-flux step is a mode step
    t = eng.step(30)
    m = eng.modes()
    assert m['samples'] == 3 and m['skipped'] == 0
    assert np.array_equal(m['N'].reshape(S, M).sum(axis=1), t['N_sv'][[9, 19, 29]].sum(axis=0))
    eng.set_modes(20)
    eng.step(40)
    assert eng.modes()['samples'] == 2


def test_history_row_config2_full_size():
    """BASELINE config 2 at 1e7 particles: box store, alternating walk, 3072 segments, 178 746 modes x 20 subvolumes."""
    import test_gpu_fullsize as FS
    pop, geo, ph = FS.build('c2', 10000000)
    eng = pop.engine
    eng.set_modes(10)
    info = eng.modes_info()
    print('config 2: mode tally %d bytes, owner path %d, k_E %d' % (info['bytes'], info['owner_path'], info['k_E']))
    assert info['owner_path'] == 1
    t = eng.step(10)
    m = eng.modes(reset=True)
    assert m['samples'] == 1 and m['skipped'] == 0
    ct = dict(centers=np.zeros((eng.S, 3)), tables=dict(group_vel=ph.group_vel))
    check_against_row(m, t, 9, ct, eng.modes_info(), label='(config 2, 1e7)')
    assert m['N'].sum() == t['N_sv'][9].sum() == eng.timing()['live']


def test_history_row_wire():
    """The 5000-face STL wire (split sweep, k_events, rough facets with migration)."""
    import bench
    from nanokappa_amd import synthetic
    from nanokappa_amd.phonon import Phonon
    from nanokappa_amd.population import Population
    args, geo = bench.wire_geometry(200000)
    ph = Phonon(args, 0, material=synthetic.make_material(9, 'Si', temperatures=np.arange(200.0, 401.0, 10.0)))
    pop = bench.quiet(Population, args, geo, ph)
    eng = pop.engine
    eng.set_modes(10)
    ct = dict(centers=np.zeros((eng.S, 3)), tables=dict(group_vel=ph.group_vel))
    seen = 0
    for call in range(2):
        halts0 = eng.timing()['halts']
        t = eng.step(10)
        m = eng.modes(reset=True)
        halted = eng.timing()['halts'] > halts0
        # a mode step is a sample unless the engine says it halted in this call (migrants that waited in an inbox while the
        # store grew): no silent skips
        assert m['samples'] == 1 or (halted and m['samples'] + m['skipped'] == 1), (m['samples'], m['skipped'], halted)
        if m['samples'] == 0:
            continue
        seen += 1
        check_against_row(m, t, 9, ct, eng.modes_info(), label='(wire)')
    assert seen >= 1


# ---------------------------------------------------------------------------------------------- 9. the band pass
@pytest.mark.parametrize('kind', ['frequency', 'permuted'])
def test_against_the_band_pass(kind):
    from nanokappa_amd import modes as MD, spectral as SP
    ct = case_tables('ttrrp')
    S, M, B = ct['centers'].shape[0], ct['M'], 100
    if kind == 'frequency':
        band = SP.frequency_bands(ct['ph'].omega, B)[0]
    else:
        rng = np.random.default_rng(17)
        band = (rng.permutation(M) % B).astype(np.int32)
        band[rng.random(M) < 0.2] = -1
    pos, mode, occ, counter = random_population(ct, 20000, seed=5)
    eng = make_engine(ct, pos, mode, occ, counter, seed=3)
    eng.set_bands(band, B)
    eng.set_modes(10)
    for call in range(2):
        t = eng.step(10)
        m = eng.modes(reset=True)
        assert m['samples'] == 1 and list(t['band_steps']) == [10 * call + 9]
        N, E = m['N'].reshape(S, M), m['E'].reshape(S, M)
        assert np.array_equal(MD.band_sums(N, band, B), t['band_N'][0])
        F = np.moveaxis(MD.band_sums(np.moveaxis(MD.mode_flux(E, vg_of(ct)), 2, 1), band, B), 1, 2)      # [S, B, 3]
        d = rel_row(F, t['band_F'][0], tag='modes banded against band_F')
        vmax = np.max(np.abs(vg_of(ct)))
        info = eng.modes_info()
        x = excess(F, t['band_F'][0], vmax * (quant_bound(t['band_N'][0], info['k_E']) + float_bound(t['band_N'][0], info['B_E']))[..., None])
        print('modes summed by band (%s) against the band pass: %.3e of the largest, %.3e beyond the rounding bound' % (kind, d, x))
        assert x <= TOL_MODES_ROW


# ---------------------------------------------------------------------------------------------- 10. state mode
def state_on_host(eng, ct, T_ref=None):
    p = eng.download()
    x, m, n = p['positions'], p['mode'].astype(int), p['occupation']
    if T_ref is None:
        T = eng.eval('interp_T', x)
        n0 = np.where(T > 0, eng.eval('occupation', T, m), 0.0)
    else:
        n0 = eng.eval('occupation', np.full(m.shape[0], T_ref), m)
    e = ct['ph'].hbar * ct['ph'].omega.ravel()[m] * (n - n0)
    return eng.classify(x).astype(int), m, e


@pytest.mark.parametrize('case,T_ref', [('ttp', None), ('ttrrp', None), ('ttp', 300.0)])
def test_state_mode_against_host(case, T_ref):
    from nanokappa_amd import modes as MD
    ct = case_tables(case)
    S, M = ct['centers'].shape[0], ct['M']
    pos, mode, occ, counter = random_population(ct, 20000, seed=12, T0=303.0)     # 5 K above the subvolumes: e_i of full size
    eng = make_engine(ct, pos, mode, occ, counter, seed=2)
    if T_ref is not None:
        eng.set_params(dt=1.0, particle_density=ct['particle_density'], T_ref=T_ref, flux_every=10, contains_every=100, track_ids=True)
    eng.set_modes(10)
    eng.step(7)
    st = eng.tally_modes_state()
    sv, m, e = state_on_host(eng, ct, T_ref)
    q = MD.quantised(sv, m, e, S, M, st['k_E'])
    assert st['N_raw'].sum() == sv.shape[0] == eng.timing()['live']
    assert np.array_equal(st['N_raw'].reshape(S, M), q['N_raw'])
    du = int(np.max(np.abs(st['E_raw'].reshape(S, M) - q['E_raw'])))
    print('state mode %s: device integers against host integers: %d units' % (case, du))
    rel_row(st['E'].reshape(S, M), q['E'], tag='modes state integers against the host integers', bound=0.0)
    assert du == 0
    assert np.abs(st['E_raw']).max() > 0
    ref = MD.table_from_particles(sv, m, e, S, M)
    assert np.all(np.abs(st['E'].reshape(S, M) - ref['E']) <= quant_bound(ref['N'], st['k_E']) + ref['N'] * np.ldexp(np.max(np.abs(e)), -53))


# ---------------------------------------------------------------------------------------------- 11. the reference itself
def test_state_mode_against_reference_golden():
    """The reference's own Visualisation.flux_contribution on the post-step state of step.npz (tests/golden/k_contribution.npz):
    that state uploaded with its subvolume temperatures, mode_k of the state-mode table summed into the reference's 100
    frequency bins."""
    from util import golden, sub, golden_phonon
    from nanokappa_amd import modes as MD, spectral as SP
    from nanokappa_amd.engine import Engine
    from nanokappa_amd.constants import Constants
    K = Constants()
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
    eng.set_modes(1)
    st = eng.tally_modes_state()
    band, edges = SP.frequency_bands(ph.omega, 100)
    assert np.array_equal(edges, kc['bins'])
    km = MD.mode_k(st['E'], st['N'], ph.group_vel, kc['subvol_connections'], kc['subvol_con_vectors'], kc['mean_T'],
                   int(kc['number_of_active_modes']), ph.number_of_qpoints * ph.volume_unitcell, K.eVpsa2_in_Wm2, K.a_in_m)
    k = MD.band_sums(km, band, 100)
    y = kc['y']
    d = rel_row(k, y, tag='modes k(omega) against the reference golden', bound=TOL_MODES_K_GOLDEN)
    print('state mode against the reference golden: largest deviation %.3e of max |k|' % d)
    assert d <= TOL_MODES_K_GOLDEN


# ---------------------------------------------------------------------------------------------- 12. paths, splits, reruns
def _run_modes(ct, pop4, flags=0, nsteps=30, seed=3):
    pos, mode, occ, counter = pop4
    eng = make_engine(ct, pos, mode, occ, counter, seed=seed)
    eng.set_modes(10, flags=flags)
    eng.step(nsteps)
    m = eng.modes()
    st = eng.tally_modes_state()
    return m, st, eng.modes_info()


def test_identical_bits_across_runs_and_paths(monkeypatch):
    from nanokappa_amd.engine import MODES_GLOBAL
    ct = case_tables('ttrrp')
    pop4 = random_population(ct, 20000, seed=21)
    runs = [_run_modes(ct, pop4), _run_modes(ct, pop4), _run_modes(ct, pop4, flags=MODES_GLOBAL)]
    monkeypatch.setenv('NK_MODES_PATH', 'global')
    runs.append(_run_modes(ct, pop4))
    assert [r[2]['owner_path'] for r in runs] == [1, 1, 0, 0]
    for r in runs[1:]:
        assert r[0]['samples'] == runs[0][0]['samples'] == 3 and r[0]['skipped'] == 0
        for k in ('N', 'E'):
            assert r[0][k].tobytes() == runs[0][0][k].tobytes(), k
        assert r[1]['N_raw'].tobytes() == runs[0][1]['N_raw'].tobytes() and r[1]['E_raw'].tobytes() == runs[0][1]['E_raw'].tobytes()
    assert np.abs(runs[0][0]['E']).max() > 0


def test_no_partition_takes_the_global_path(monkeypatch):
    """NK_NO_PARTITION=1 (developer probe: a stored index is the mode itself, nobody owns a row): the global path is chosen by
    itself and gives the owner path's bytes.  (test_gpu_parity.py::test_multistep_vs_oracle[ttp-*] passes under that variable,
    which is what makes it fit for a test: DESIGN.md, "Mode-resolved tally".)"""
    ct = case_tables('ttp')
    pop4 = random_population(ct, 20000, seed=21)
    r0 = _run_modes(ct, pop4)
    monkeypatch.setenv('NK_NO_PARTITION', '1')
    r1 = _run_modes(ct, pop4)
    assert r0[2]['owner_path'] == 1 and r1[2]['owner_path'] == 0
    assert r0[0]['samples'] == r1[0]['samples'] == 3 and r1[0]['skipped'] == 0
    for k in ('N', 'E'):
        assert r0[0][k].tobytes() == r1[0][k].tobytes(), k
    assert r0[1]['N_raw'].tobytes() == r1[1]['N_raw'].tobytes() and r0[1]['E_raw'].tobytes() == r1[1]['E_raw'].tobytes()


def test_split_of_the_particles_does_not_change_the_integers():
    """Two engine contexts holding the two halves of an ensemble (one capacity, so one k_E): their integers add up to the
    whole's, bit for bit -- what the integer all-reduce over ranks relies on."""
    ct = case_tables('ttp')
    pos, mode, occ, counter = random_population(ct, 30000, seed=31, T0=303.0)
    cut = 11000
    out = []
    for sl, off in [(slice(0, cut), 0), (slice(cut, None), cut), (slice(None), 0)]:
        eng = make_engine(ct, pos[sl], mode[sl], occ[sl], counter, seed=2, pid_offset=off)
        eng.set_modes(10, capacity=1 << 20)
        out.append((eng.tally_modes_state(), eng.modes_info()))
    (a, ia), (b, ib), (c, ic) = out
    assert ia['k_E'] == ib['k_E'] == ic['k_E'] and ia['capacity'] == ib['capacity'] == ic['capacity'] == 1 << 20
    assert a['N_raw'].sum() == cut and b['N_raw'].sum() == 30000 - cut
    assert np.array_equal(a['N_raw'] + b['N_raw'], c['N_raw']) and np.array_equal(a['E_raw'] + b['E_raw'], c['E_raw'])
    assert np.abs(c['E_raw']).max() > 0


# ---------------------------------------------------------------------------------------------- 13. a store that regrows
@pytest.mark.parametrize('case', ['ttp', 'ttrrp'])
def test_store_regrows_in_mid_window(case, monkeypatch):
    """Six times the entry rate into a store with hardly any head room: the segmentation changes in mid-window, the table is
    indexed by the global mode and does not; the accumulated table equals the per-sample oracle sums added up; steps of a
    halted batch are walked again and are samples once."""
    from nanokappa_amd import modes as MD
    monkeypatch.setenv('NK_TIGHT_STORE', '1')
    ct = case_tables(case)
    S, M = ct['centers'].shape[0], ct['M']
    pos, mode, occ, counter = random_population(ct, 20000, seed=9)
    sim = make_oracle_sim(ct, pos, mode, occ, counter, seed=3, cap=600000, emit_scale=6.0)
    eng = make_engine(ct, pos, mode, occ, counter, seed=3, emit_scale=6.0)
    same_event_rule(eng, sim)
    eng.set_modes(10)
    slots0 = eng.timing()['slots']
    eng.step(60)
    m = eng.modes()
    assert eng.timing()['slots'] > slots0 and eng.timing()['regrows'] > 0
    N0, E0, nq = np.zeros((S, M)), np.zeros((S, M)), np.zeros((S, M))
    for s in range(60):
        sim.run_timestep()
        if (s + 1) % 10 == 0:
            P = sim.P
            k = P.N
            r = MD.table_from_particles(P.sv[:k].astype(int), P.mode[:k].astype(int), P.energy[:k], S, M)
            N0 += r['N']
            E0 += r['E']
    # a sample is dropped only where migrants waited in an inbox while the store grew: then it is counted in `skipped`
    assert m['samples'] + m['skipped'] == 6
    if m['skipped'] == 0:
        N, E = m['N'].reshape(S, M), m['E'].reshape(S, M)
        assert np.array_equal(N, N0)
        d = rel_row(E, E0, tag='modes E against the oracle, regrown store')
        x = excess(E, E0, quant_bound(N0, eng.modes_info()['k_E']))
        print('regrown store %s: largest deviation %.3e of the largest bin, %.3e beyond the rounding bound' % (case, d, x))
        assert x <= TOL_MODES_ORACLE
    else:
        assert case == 'ttrrp'


# ---------------------------------------------------------------------------------------------- 14. nothing else moves
@pytest.mark.parametrize('case,gen', [('ttp', 0), ('ttrrp', 0), ('ttp', 2)])
def test_modes_leave_everything_else(case, gen):
    ct = case_tables(case)
    pos, mode, occ, counter = random_population(ct, 20000, seed=8)
    runs = []
    for on in (False, True):
        eng = make_engine(ct, pos, mode, occ, counter, seed=4, gen=gen)
        if on:
            eng.set_modes(10)
        else:
            info = eng.modes_info()
            assert info['on'] == 0 and info['bytes'] == 0
        t = eng.step(25)
        runs.append((t, eng.download()))
        if on:
            eng.set_modes(0)
            assert eng.modes_info()['bytes'] == 0 and eng.modes_info()['on'] == 0
            eng.step(5)
    (t0, p0), (t1, p1) = runs
    assert sorted(t0) == sorted(t1)
    assert_runs_equal(t0, t1)
    i0, i1 = np.argsort(p0['pid']), np.argsort(p1['pid'])
    assert np.array_equal(p0['pid'][i0], p1['pid'][i1])
    assert np.array_equal(p0['mode'][i0], p1['mode'][i1])
    assert allclose(p0['positions'][i0], p1['positions'][i1], rtol=0, atol=TOL_X)
    assert allclose(p0['occupation'][i0], p1['occupation'][i1], rtol=TOL_OCC, atol=0)


# ---------------------------------------------------------------------------------------------- 15. error paths
def test_error_paths():
    from nanokappa_amd.engine import Engine, NkError, MODES_TEST_SMALL_BOUND
    ct = case_tables('ttp')
    S, M = ct['centers'].shape[0], ct['M']
    pos, mode, occ, counter = random_population(ct, 5000, seed=8, T0=303.0)
    eng = make_engine(ct, pos, mode, occ, counter, seed=4)                  # flux_every = 10
    for every in (-10, 15, 5):
        with pytest.raises(NkError, match='multiple of flux_every'):
            eng.set_modes(every)
    assert eng.modes_info()['on'] == 0
    with pytest.raises(NkError, match='off'):
        eng.modes()
    bare = Engine(0, 1)
    with pytest.raises(NkError, match='material'):
        bare.set_modes(10)
    # a bound 2^40 times too small: every ordinary term exceeds it -- an error that names the sum, never wrapped integers
    eng.set_modes(10, flags=MODES_TEST_SMALL_BOUND)
    with pytest.raises(NkError, match='overflow.*of E above B_E'):
        eng.tally_modes_state()
    with pytest.raises(NkError, match='overflow.*of E above B_E'):
        eng.step(10)
    m = eng.modes()                                                          # the table was left without the offending terms
    assert m['N'].sum() == eng.timing()['live'] and np.max(np.abs(m['E'])) <= 5000 * eng.modes_info()['B_E']
    # ... and the engine is usable afterwards
    eng.set_modes(10)
    eng.step(10)
    assert eng.modes()['samples'] == 1


# ---------------------------------------------------------------------------------------------- 16. communicator
def test_modes_through_single_rank_communicator(monkeypatch):
    from nanokappa_amd.engine import comm_unique_id
    ct = case_tables('ttp')
    pos, mode, occ, counter = random_population(ct, 20000, seed=9)
    ref = make_engine(ct, pos, mode, occ, counter, seed=1)
    ref.set_modes(10)
    ref.step(20)
    m0, s0 = ref.modes(), ref.tally_modes_state()
    monkeypatch.setenv('NK_FORCE_COMM', '1')
    eng = make_engine(ct, pos, mode, occ, counter, seed=1)
    eng.comm_init(comm_unique_id(), 0, 1)
    eng.set_modes(10)
    eng.step(20)
    m1, s1 = eng.modes(), eng.tally_modes_state()
    assert m0['samples'] == m1['samples'] == 2 and m0['skipped'] == m1['skipped'] == 0
    for k in ('N', 'E'):
        assert m0[k].tobytes() == m1[k].tobytes(), k
    assert s0['N_raw'].tobytes() == s1['N_raw'].tobytes() and s0['E_raw'].tobytes() == s1['E_raw'].tobytes()


# ---------------------------------------------------------------------------------------------- 17. Population
def test_population_end_to_end(tmp_path):
    """A parameter-file run of config 2 with --mode_tally 10 --n_mean 5 writes k_accumulation.txt (and its frequency twin) and
    mode_tally.npz beside the other outputs; they hold what Population.mode_distribution() / kappa_accumulation() return."""
    import bench
    from nanokappa_amd import nanokappa, modes as MD
    argv, species, _ = bench.config_argv('c2', 100000, 200.0)
    argv = argv + ['--seed', '7', '--mode_tally', '10', '--iterations', '120', '--results_folder', str(tmp_path / 'run'), '--n_mean', '5']
    pf = tmp_path / 'params.txt'
    pf.write_text(' '.join(argv))
    cwd = os.getcwd()
    os.chdir(str(tmp_path))
    try:
        pop = nanokappa.main(['-ff', str(pf)])
    finally:
        sys.stdout = sys.__stdout__
        os.chdir(cwd)
    folder = pop.results_folder_name
    for by in ('mfp', 'frequency'):
        assert os.path.exists(MD.k_accumulation_path(folder, by))
    z = MD.read_mode_tally(MD.mode_tally_path(folder))
    d = pop.mode_distribution()
    # n_mean = 5 rows of 10 steps, every = 10: windows of 50 steps.  After 120 steps the latest complete window is steps
    # 51..100: exactly its five mode steps, whatever came after
    assert pop.modes_window == 50 and d['samples'] == 5 == int(z['samples']) and d['step'] == 100 == int(z['step'])
    assert pop.engine.modes()['samples'] == 2                   # (steps 110 and 120 of the window in progress)
    assert np.array_equal(z['N'], d['N']) and np.array_equal(z['E'], d['E']) and z['N'].shape == (pop.n_of_subvols,) + pop._ph.omega.shape
    assert abs(d['N'].sum() / 5 - pop.N_p) <= 0.02 * pop.N_p
    km = pop.mode_k()
    for by in ('mfp', 'frequency'):
        a = pop.kappa_accumulation(by)
        g, c = MD.read_k_accumulation(MD.k_accumulation_path(folder, by))
        assert np.array_equal(g, a['grid']) and np.array_equal(c, a['k'])
        # the last accumulation point is the sum of mode_k (two orders of one float sum: M 2^-52 sum |k_m|)
        tot = np.nan_to_num(km).sum(axis=1)
        assert np.all(np.abs(c[:, -1] - tot) <= km.shape[1] * np.ldexp(1.0, -52) * np.abs(np.nan_to_num(km)).sum(axis=1))
        assert np.all(np.diff(g) > 0)
    assert np.all(np.isfinite(km)) and np.abs(km).max() > 0
    pop.set_modes(0)
    assert pop.engine.modes_info()['bytes'] == 0
    pop.run(10)


def _modes_pop(extra=()):
    import bench
    from nanokappa_amd import synthetic
    from nanokappa_amd.argument_parser import initialise_parser
    from nanokappa_amd.geometry import Geometry
    from nanokappa_amd.phonon import Phonon
    from nanokappa_amd.population import Population
    argv, species, _ = bench.config_argv('c2', 50000, 200.0)
    args = initialise_parser().parse_args(argv + ['--seed', '11', '--n_mean', '3', '--mode_tally', '10'] + list(extra))
    args.results_folder = ''
    geo = bench.quiet(Geometry, args)
    ph = Phonon(args, 0, material=synthetic.make_material(31, species, temperatures=np.arange(200.0, 401.0, 10.0)))
    return bench.quiet(Population, args, geo, ph)


def test_window_reproduces_the_band_sums():
    """--spectral_bands 100 in the same run: the window's mode table banded on the host is the sum of the window's band rows."""
    import bench
    from nanokappa_amd import modes as MD
    pop = _modes_pop(['--spectral_bands', '100'])
    assert pop.modes_window == 30 and pop.n_bands == 100
    B, S = pop.n_bands, pop.n_of_subvols
    bF, bN = np.zeros((S, B, 3)), np.zeros((S, B))
    for _ in range(3):
        bench.quiet(pop.run, 10)
        bF += pop.conv_rows[-1]['band_F']                       # (the convergence row of this step keeps its band sums)
        bN += pop.conv_rows[-1]['band_N']
    d = pop.mode_distribution()
    assert d['samples'] == 3 and d['step'] == 30
    info = pop.engine.modes_info()
    N, E = d['N'].reshape(S, -1), d['E'].reshape(S, -1)
    assert np.array_equal(MD.band_sums(N, pop.band_of_mode, B), bN)
    vg = np.asarray(pop._ph.group_vel).reshape(-1, 3)
    F = np.moveaxis(MD.band_sums(np.moveaxis(MD.mode_flux(E, vg), 2, 1), pop.band_of_mode, B), 1, 2)
    x = excess(F, bF, np.max(np.abs(vg)) * (quant_bound(bN, info['k_E']) + float_bound(bN, info['B_E']))[..., None])
    print('window banded on the host against the window\'s band rows: %.3e beyond the derived bound' % x)
    assert x <= TOL_MODES_ROW


def test_window_does_not_depend_on_how_the_run_is_cut():
    """run(70) in one go, step by step, and in uneven pieces: the same windows (30 steps: 3 rows), the same sample counts, the
    same counts per bin; the reals as two runs of the engine agree (their tallies are summed in different orders)."""
    import bench
    from util import TOL_T
    out = []
    for pieces in ([70], [1] * 70, [7, 13, 29, 21]):
        pop = _modes_pop()
        assert pop.modes_window == 30
        for k in pieces:
            bench.quiet(pop.run, k)
        out.append((pop.mode_distribution(), pop.engine.modes(), pop.engine.modes_info()))
    d0, r0, i0 = out[0]
    assert d0['samples'] == 3 and d0['step'] == 60 and r0['samples'] == 1      # window 31..60 complete; step 70 in progress
    for d, r, i in out[1:]:
        assert d['samples'] == d0['samples'] and d['step'] == d0['step'] and r['samples'] == r0['samples']
        assert np.array_equal(d['N'], d0['N']) and np.array_equal(r['N'], r0['N'])
        # (a term is C_i (T_i - T_sv) with differences of the order of 1 K, and two runs' T_sv agree to TOL_T kelvin: TOL_T of
        # the largest bin, as the field's counterpart of this test holds its heat flux; plus the rounding of both sides)
        lim = 2 * quant_bound(d0['N'], min(i['k_E'], i0['k_E'])) + TOL_T * np.max(np.abs(d0['E']))
        assert np.all(np.abs(d['E'] - d0['E']) <= lim)
