"""Kinetic flights on the GPU (Engine.kinetic_flights; k_kinetic) against their CPU restatement (tests/kinetic_cases.py), ray by
ray; the ballistic limit, telescoping, the isothermal identity, reciprocity and flux conservation on the engine's own rays;
determinism and non-interference; the refusals; Population.kinetic_flights and --kinetic.

Tolerances of the per-ray comparisons: <= 10 x the largest deviation measured on an MI355X (profiles/kinetic_margins.txt; recorded
by tests/util.py at every call site), the project's rule.  A ray's displacement is a sum of t v over its segments whose components
cancel after scatterings, so it is compared absolutely (angstrom); its dwell time relative to itself."""
import os
import sys

import numpy as np
import pytest

import kinetic_cases as K
import free_path_cases as FC
from nanokappa_amd import kinetic as KN
from util import allclose, rel_err, make_engine, random_population

pytestmark = pytest.mark.gpu

# Per ray, kernel against restatement: every segment adds t v with one rounding (a fused multiply-add on the device, Dekker's
# emulation in NumPy) and t = -tau ln(u) carries the device logarithm's last bit.  Measured on an MI355X
# (profiles/kinetic_margins.txt): D 5.7e-14 ('ttp'), 1.14e-13 ('ttp_16'), 4.3e-14 ('ttrrp_k'), 2.47e-13 ('wire72', 500 A long);
# dwell 1.85e-16 .. 3.3e-16.
TOL_RAY_D = {'ttp': 5e-13, 'ttp_16': 1e-12, 'ttrrp_k': 4e-13, 'wire72': 2.4e-12}    # angstrom
TOL_RAY_DWELL = 1.8e-15                                                               # relative
TOL_TELESCOPE = {'ttp': 5e-13, 'ttp_16': 1e-12}   # angstrom: |D_x - (+-L or 0)|, the same sums (measured 5.7e-14, 1.02e-13)
_ENG = {}


def engine(case):
    """One engine per case for the whole module (the calls keep nothing on the device)."""
    if case not in _ENG:
        _ENG[case] = K.engine_for(K.case(case), seed=99)          # (the calls' seeds are given: the engine's must not matter)
    return _ENG[case]


def call(case, scale, n, seed, **kw):
    ct = K.case(case)
    return engine(case).kinetic_flights(K.lifetimes(ct, scale), K.heat_capacity(ct), n=n, seed=seed, **kw)


def stat_calls(name):
    p = K.STAT[name]
    return FC.cached(('kin_gpu_stat', name), lambda: [call(p['case'], p['scale'], p['n'], s) for s in p['seeds']])


def host_rows(r):
    """A source's row from the per-ray outputs at the report's scales: the sums the device adds as integers."""
    rep = r['report']
    F = r['ends'].shape[0]
    rows = np.zeros((F, 32), dtype=np.int64)
    Bx, Bt = rep['B_x'], rep['B_t']
    for f in range(F):
        e = r['ray_end'][f]
        rows[f, :F] = [(e == g).sum() for g in range(F)]
        rows[f, 8:11] = [(e == c).sum() for c in (-1, -2, -3)]
        rows[f, 11], rows[f, 12] = r['ray_events'][f].sum(), r['ray_casts'][f].sum()
        D, T = r['ray_D'][f], r['ray_dwell'][f]
        assert np.abs(D).max() <= 32.0 * Bx and T.max() <= 1024.0 * Bt                 # no term is left out
        rows[f, 13:16] = np.rint(D * 2.0 ** rep['k_D']).astype(np.int64).sum(axis=0)
        rows[f, 16:19] = np.rint(D * D * 2.0 ** rep['k_D2']).astype(np.int64).sum(axis=0)
        rows[f, 19] = np.rint(T * 2.0 ** rep['k_T']).astype(np.int64).sum()
    return rows


@pytest.mark.parametrize('name', ['ttp', 'ttp_16', 'ttrrp_k', 'wire72'])
def test_rays_against_restatement(name):
    p = K.PARITY[name]
    ref, other = K.parity_run(name), K.parity_run(name, fused=False)
    got = call(p['case'], p['scale'], K.PARITY_N, p['seed'], rays=True)
    keep = ref['ray_hash'] == other['ray_hash']       # rays whose events hinge on the rounding of a hit point are left out
    left_out = 1.0 - keep.mean()
    print('%s: %d rays, %.4f %% left out, %d events' % (name, keep.size, 100 * left_out, got['report']['events']))
    assert left_out <= FC.MAX_OTHER_SEQUENCE and got['report']['overflow'] == 0
    assert np.array_equal(got['ray_x0'], ref['ray_x0']) and np.array_equal(got['ray_mode'], ref['ray_mode'])
    for k in ('ray_end', 'ray_events', 'ray_casts', 'ray_hash'):
        assert np.array_equal(got[k][keep], ref[k][keep]), k
    assert allclose(got['ray_D'][keep], ref['ray_D'][keep], rtol=0, atol=TOL_RAY_D[name], tag=name + ' D'), 'displacements differ'
    assert rel_err(got['ray_dwell'][keep], ref['ray_dwell'][keep], tag=name + ' dwell', bound=TOL_RAY_DWELL) <= TOL_RAY_DWELL
    # the integer tallies: the host's sums of the per-ray values at the same scales, bit for bit; the per-subvolume words against
    # the restatement's (every ray kept: the same segments, the same terms)
    assert np.array_equal(got['rows'], host_rows(got))
    for k in ('k_t', 'k_x', 'k_T', 'k_D', 'k_D2', 'B_t', 'B_x'):
        assert got['report'][k] == ref['report'][k], k
    assert np.array_equal(got['sub'][:, :, 0].sum(axis=1) > 0, [True, True])
    if keep.all():
        assert np.array_equal(got['ends'], ref['ends'])
        d = np.abs(got['sub'] - ref['sub'])
        # a term differs by one unit where the device's t rounds the other way; never by more per segment
        assert d.max() <= got['report']['events'] and np.array_equal(got['sub'] != 0, ref['sub'] != 0)


def test_ballistic_limit():
    ct = K.case('ttp')
    r = call('ttp', np.inf, 256, 51)
    assert np.array_equal(r['ends'], [[0, 256], [256, 0]]) and np.array_equal(r['events'], r['casts'])
    c, tau, v = K.heat_capacity(ct), K.lifetimes(ct, np.inf), FC.group_vel(ct)
    src, area, n_in, cen = K.source_geometry(ct)
    s = KN.summarise(r, c, v, tau, 300.0, area, n_in, [302.0, 298.0], ct['volumes'], pair=KN.parallel_pair(np.arange(2), -n_in, area, cen))
    lv = KN.live_modes(c, tau)
    want = 200.0 * 200.0 * np.sum((c * np.maximum(v[:, 0], 0))[lv]) * KN.watt()
    assert s['transmission'][0, 1] == 1.0 and rel_err(s['G'][0, 1], want, tag='ballistic G', bound=1e-12) <= 1e-12


@pytest.mark.parametrize('name', ['ttp', 'ttp_16'])
def test_telescoping_and_counts(name):
    p = K.PARITY[name]
    r = call(p['case'], p['scale'], K.PARITY_N, p['seed'], rays=True)
    assert np.array_equal(r['ends'].sum(axis=1) + r['lost'] + r['missed'] + r['capped'], [K.PARITY_N] * 2)
    want = np.where(r['ray_end'] == 1 - np.arange(2)[:, None], 200.0 * np.array([1.0, -1.0])[:, None], 0.0)
    assert allclose(r['ray_D'][..., 0], want, rtol=0, atol=TOL_TELESCOPE[name], tag=name + ' telescope')


@pytest.mark.parametrize('name', ['ttp_16', 'box3'])
def test_isothermal_identity(name):
    ct, tau = K.stat_inputs(name)
    z, se, zq = K.isothermal_deviation(stat_calls(name), ct, tau)
    print('%s: mean dT - 1 at most %.2f standard errors, largest standard error %.4f, q at most %.2f' % (name, z, se, zq))
    assert se < 0.02 and z <= 5.0 and zq <= 5.0


def test_reciprocity():
    ct, tau = K.stat_inputs('box3')
    z = K.reciprocity_deviation(stat_calls('box3'), ct, tau)
    print('G_fg - G_gf at most %.2f standard errors' % z)
    assert z <= 5.0


def test_flux_conservation():
    ct, tau = K.stat_inputs('ttp_16')
    z, zo, rel = K.flux_deviation(stat_calls('ttp_16'), ct, tau)
    print('q_x - G dT / A at most %.2f standard errors (%.3f of the flux each), q_y, q_z at most %.2f' % (z, rel, zo))
    assert z <= 5.0 and zo <= 5.0


def test_determinism_grid_and_other_calls():
    p = K.PARITY['ttp_16']
    keys = ('rows', 'sub', 'ray_x0', 'ray_mode', 'ray_end', 'ray_events', 'ray_casts', 'ray_D', 'ray_dwell', 'ray_hash')
    a = call('ttp', p['scale'], 300, p['seed'], rays=True)
    assert a['report']['grid'] == 1 and a['report']['lds_bins'] == 1
    small = call('ttp', p['scale'], 100, p['seed'], rays=True)                      # another N in between
    b = call('ttp', p['scale'], 300, p['seed'], rays=True)
    g = call('ttp', p['scale'], 300, p['seed'], rays=True, rays_per_wave=64)        # 10 waves in 3 workgroups instead of 2 in 1
    m = call('ttp', p['scale'], 300, p['seed'], rays=True, lds_bins=False)          # the words straight to memory
    assert g['report']['grid'] == 3 and m['report']['lds_bins'] == 0
    for k in keys:
        assert np.array_equal(a[k], b[k]) and np.array_equal(a[k], g[k]) and np.array_equal(a[k], m[k]), k
    for k in keys[2:]:                                                              # a ray does not depend on the call's N
        assert np.array_equal(small[k], a[k][:, :100]), k
    assert not np.array_equal(call('ttp', p['scale'], 300, p['seed'] + 1)['rows'], a['rows'])


def test_does_not_interfere_with_the_steps():
    """20 steps with a call after step 10 against 20 steps without (tests/test_gpu_free_path.py states what is compared how)."""
    from test_gpu_replicas import assert_same_rows, assert_same_particles
    ct = K.case('ttp')
    pos, mode, occ, counter = random_population(ct, 30000, seed=5)
    engs, rows = [], []
    for with_call in (False, True):
        eng = make_engine(ct, pos, mode, occ, counter, seed=42)
        t0 = eng.step(10)
        if with_call:
            r = eng.kinetic_flights(K.lifetimes(ct), K.heat_capacity(ct), n=500, seed=3)
            assert r['report']['rays'] == 1000 and eng.get_step() == 10
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
    from test_gpu_free_path import fp_engine
    ct = K.case('ttp')
    tau, c = K.lifetimes(ct), K.heat_capacity(ct)

    def refused(eng, text, code=r'\(-2\)', **kw):
        args = dict(tau=tau, c=c, n=8)
        args.update(kw)
        with pytest.raises(NkError, match=code) as e:
            eng.kinetic_flights(args.pop('tau'), args.pop('c'), **args)
        assert text in str(e.value), str(e.value)

    def with_bc(case, bc, rough=True):
        g = dict(case['mesh'])
        g['bound_cond'] = np.array(bc)
        return fp_engine(dict(case, mesh=g), rough=rough)

    eng = Engine(0, 1)
    eng.set_material(ct['tables'])
    refused(eng, 'no mesh')
    eng.close()
    eng = fp_engine(ct)
    refused(eng, 'n_samples', n=0)
    refused(eng, 'n_samples', n=-3)
    refused(eng, 'entries', code='kinetic_flights', tau=tau[:-1])
    refused(eng, 'entries', code='kinetic_flights', c=np.concatenate([c, c]))
    refused(eng, 'no live mode', code='kinetic_flights', c=np.zeros_like(c))
    assert eng.kinetic_flights(tau, c, n=8)['report']['calls'] == 1                  # nothing ran before
    eng.close()
    eng = with_bc(ct, ['T', 'F', 'P', 'P', 'P', 'P'])
    refused(eng, "'F'")
    eng.close()
    eng = with_bc(ct, ['R', 'R', 'P', 'P', 'P', 'P'], rough=False)
    refused(eng, "no facet with boundary condition 'T'")
    eng.close()
    cw = K.case('wire72')
    bc = ['R'] * int(len(cw['mesh']['bound_cond']))
    for f in range(9):
        bc[f] = 'T'
    eng = with_bc(cw, bc, rough=False)          # (the ninth source is met before the first rough facet)
    refused(eng, 'more than 8 facets')
    eng.close()
    eng = fp_engine(K.case('ttrrp_k'), rough=False)
    refused(eng, 'rough')
    eng.close()


def test_population_and_front_end(tmp_path):
    """--kinetic 512 on 'ttp' writes k_kinetic.txt and kinetic.npz before the first step, with the numbers of the engine call;
    Population.kinetic_flights returns them; k_kinetic.txt round-trips; without the option no file is written."""
    from nanokappa_amd import nanokappa
    from test_gpu_free_path import _ttp_argv

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

    pop = run('with', ['--kinetic', '512'])
    folder = pop.results_folder_name
    assert os.path.exists(KN.k_kinetic_path(folder)) and os.path.exists(KN.kinetic_npz_path(folder))
    s = pop.kinetic_last
    assert s['T'] == 300.0 and s['n'] == 512 and s['axis'] == 0 and s['L'] == 200.0 and list(s['T_f']) == [302.0, 298.0]
    # (no order between the free-path estimate and kappa_eff: on this box the estimate lies above the solution)
    assert 0 < s['kappa_eff'] < s['kappa_bulk'] and 0 < s['kappa_free_path'] < s['kappa_bulk'] and s['ends'].sum() == 1024
    assert abs(s['kappa_eff'] / s['kappa_free_path'] - 1) < 0.2 and s['kappa_eff_se'] < 0.05 * s['kappa_eff']
    txt, z = KN.read_k_kinetic(KN.k_kinetic_path(folder)), KN.read_kinetic_npz(KN.kinetic_npz_path(folder))
    for k in ('G', 'G_se', 'g', 'T_f', 'events', 'casts'):
        assert np.array_equal(txt[k], s[k]), k
    assert txt['kappa_eff'] == s['kappa_eff'] and txt['kappa_bulk'] == s['kappa_bulk'] and txt['N'] == 512
    for k in ('transmission', 'dT', 'q', 'dwell'):
        assert np.array_equal(z[k], s[k]), k
    again = pop.kinetic_flights(n=512, write=False)                                 # the same call again: same seed, same bits
    assert np.array_equal(again['ends'], s['ends']) and np.array_equal(again['dwell'], s['dwell'])
    t = pop.kinetic_flights(n=64, T=250.0, max_events=50, write=False)
    assert t['T'] == 250.0 and t['n'] == 64 and pop.current_timestep == 10
    pop.engine.close()
    pop = run('without', [])
    folder = pop.results_folder_name
    assert not os.path.exists(KN.k_kinetic_path(folder)) and not os.path.exists(KN.kinetic_npz_path(folder))
    pop.engine.close()
