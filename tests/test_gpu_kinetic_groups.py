"""Kinetic groups on the GPU (Engine.kinetic_flights(groups=...); nk_kinetic_flights_groups, k_kinetic<GEOM, BINS, true> and
k_kinetic_fold) against the grouped CPU restatement (tests/kinetic_group_cases.py): the columns add up to the ungrouped words bit
for bit and everything else is the ungrouped call's; the columns follow the table; the LDS and the memory path give the same bits;
the ballistic limit exactly; the per-group isothermal identity on the engine's own rays; the refusals; Population.kinetic_flights
with groups and batches, and --kinetic_groups.

Against the restatement a group word is held to the rule test_gpu_kinetic.py applies to `sub`: the same nonzero pattern and at
most one unit per segment (where the device logarithm's last bit rounds t the other way), so |difference| <= the call's events;
the largest difference seen is recorded by tests/util.py (profiles/kinetic_margins.txt)."""
import os
import sys

import numpy as np
import pytest

import kinetic_cases as K
import kinetic_group_cases as KGC
import free_path_cases as FC
import test_gpu_kinetic as TK
from nanokappa_amd import kinetic as KN
from nanokappa_amd import kinetic_groups as KG
from util import allclose, make_engine, random_population

pytestmark = pytest.mark.gpu

PLAIN_KEYS = ('rows', 'sub', 'ray_x0', 'ray_mode', 'ray_end', 'ray_events', 'ray_casts', 'ray_D', 'ray_dwell', 'ray_hash')


def plain_parity_call(name):
    p = K.PARITY[name]
    return FC.cached(('kin_grp_gpu_plain', name), lambda: TK.call(p['case'], p['scale'], K.PARITY_N, p['seed'], rays=True))


def ttp_tables():
    """'ttp' with the lifetimes of 'ttp_16': (tau, the frequency table of 4 groups)."""
    ct = K.case('ttp')
    tau = K.lifetimes(ct, 1.0 / 16.0)
    return ct, tau, KGC.table_for(ct, 'frequency', 4, tau)[0]


def assert_columns_sum(r):
    assert np.array_equal(r['grp'].sum(axis=2), r['sub'])
    rep = r['report']
    assert np.array_equal(r['dwell_g'], r['grp'][..., 0] * 2.0 ** -rep['k_t']) and np.array_equal(r['flux_g'], r['grp'][..., 1:4] * 2.0 ** -rep['k_x'])


@pytest.mark.parametrize('name', ['ttp', 'ttp_16', 'ttrrp_k', 'wire72'])
def test_parity(name):
    p = K.PARITY[name]
    ct = K.case(p['case'])
    tau = K.lifetimes(ct, p['scale'])
    ref, plain = KGC.parity_run(name), plain_parity_call(name)
    keep = K.parity_run(name)['ray_hash'] == K.parity_run(name, fused=False)['ray_hash']
    assert keep.all()                                       # every ray is kept on the CPU: nothing is left out of the words
    for j, (kind, G, axis) in enumerate(KGC.PARITY_TABLES[name]):
        table, G = KGC.table_for(ct, kind, G, tau, axis)
        got = TK.call(p['case'], p['scale'], K.PARITY_N, p['seed'], rays=True, groups=(G, table))
        assert got['report']['overflow'] == 0 and got['grp'].shape == plain['sub'].shape[:2] + (G + 1, 4)
        for k in PLAIN_KEYS:                                # everything an ungrouped call returns, bit for bit
            assert np.array_equal(got[k], plain[k]), k
        for k in ('k_t', 'k_x', 'k_T', 'k_D', 'k_D2', 'B_t', 'B_x', 'events', 'casts', 'grid', 'geometry_mode'):
            assert got['report'][k] == plain['report'][k], k
        assert_columns_sum(got)
        assert np.array_equal(got['ray_hash'], ref['ray_hash']) and np.array_equal(got['ends'], ref['ends'])
        want = KGC.grp_of(ref, j)
        events = got['report']['events']
        print('%s %s: largest |difference| of a group word %d (events %d)' % (name, kind, np.abs(got['grp'] - want).max(), events))
        assert np.array_equal(got['grp'] != 0, want != 0)
        assert allclose(got['grp'], want, rtol=0, atol=events, tag='%s %s group words' % (name, kind))


def test_columns_follow_the_table():
    ct, tau, t4 = ttp_tables()
    p = K.PARITY['ttp_16']
    call = lambda G, t: TK.call('ttp', p['scale'], K.PARITY_N, p['seed'], groups=(G, t))
    a = call(4, t4)
    assert_columns_sum(a)
    assert (a['grp'][:, :, :4, 0].sum(axis=(0, 1)) > 0).all()
    one = call(1, np.where(t4 >= 0, 0, -1))                 # G = 1: everything in column 0, the rest column for the -1 modes
    assert np.array_equal(one['grp'][:, :, 0], a['grp'][:, :, :4].sum(axis=2)) and np.array_equal(one['grp'][:, :, 1], a['grp'][:, :, 4])
    cut = call(1, np.where(t4 == 3, -1, np.where(t4 >= 0, 0, -1)))          # ... group 3 sent to the rest column
    assert np.array_equal(cut['grp'][:, :, 0], a['grp'][:, :, :3].sum(axis=2))
    assert np.array_equal(cut['grp'][:, :, 1], a['grp'][:, :, 3] + a['grp'][:, :, 4]) and cut['grp'][:, :, 1, 0].sum() > 0
    perm = np.array([2, 0, 3, 1])
    b = call(4, np.where(t4 >= 0, perm[np.maximum(t4, 0)], -1))
    for g in range(4):
        assert np.array_equal(b['grp'][:, :, perm[g]], a['grp'][:, :, g]), g
    assert np.array_equal(b['grp'][:, :, 4], a['grp'][:, :, 4])
    none = call(4, np.full(t4.shape, -1))                   # all -1: everything in the rest column
    assert not none['grp'][:, :, :4].any() and np.array_equal(none['grp'][:, :, 4], a['sub'])
    for r in (one, cut, b, none):
        assert np.array_equal(r['sub'], a['sub']) and np.array_equal(r['rows'], a['rows'])


def test_determinism_of_the_paths():
    ct, tau, t4 = ttp_tables()
    p = K.PARITY['ttp_16']
    call = lambda G, t, **kw: TK.call('ttp', p['scale'], 300, p['seed'], groups=(G, t), **kw)
    plain = TK.call('ttp', p['scale'], 300, p['seed'])
    a = call(4, t4)
    assert a['report']['grid'] == 1 and a['report']['lds_bins'] == 1
    g = call(4, t4, rays_per_wave=64)                       # 10 waves in 3 workgroups instead of 2 in 1
    m = call(4, t4, lds_bins=False)                         # the columns straight to memory
    mg = call(4, t4, lds_bins=False, rays_per_wave=64)
    assert g['report']['grid'] == 3 and g['report']['lds_bins'] == 1 and m['report']['lds_bins'] == 0 and mg['report']['grid'] == 3
    for r in (a, g, m, mg):
        assert np.array_equal(r['grp'], a['grp']) and np.array_equal(r['sub'], plain['sub']) and np.array_equal(r['rows'], plain['rows'])
        assert_columns_sum(r)
    # 64 groups: 2 sources x 20 subvolumes x 65 columns x 4 words x 8 bytes = 83 KB do not fit: to memory, by itself
    t64 = KGC.table_for(ct, 'frequency', 64, tau)[0]
    if not np.array_equal(np.where(t64 >= 0, t64 // 16, -1), t4):          # the builder's edges do not nest: a hand-made nested table
        t64 = np.where(t4 >= 0, t4 * 16 + np.maximum(t64, 0) % 16, -1).astype(np.int32)
    assert a['grp'].shape[1] == 20 and np.array_equal(np.where(t64 >= 0, t64 // 16, -1), t4)
    big = call(64, t64)
    bg = call(64, t64, rays_per_wave=64)
    assert big['report']['lds_bins'] == 0 and big['report']['grid'] == 1 and bg['report']['grid'] == 3 and bg['report']['lds_bins'] == 0
    assert np.array_equal(big['grp'], bg['grp'])
    for r in (big, bg):
        assert np.array_equal(r['sub'], plain['sub']) and np.array_equal(r['rows'], plain['rows'])
        assert_columns_sum(r)
    merged = np.concatenate([big['grp'][:, :, :64].reshape(2, 20, 4, 16, 4).sum(axis=3), big['grp'][:, :, 64:]], axis=2)
    assert np.array_equal(merged, a['grp'])


def test_ballistic_limit_exact():
    ct = K.case('ttp')
    tau = K.lifetimes(ct, np.inf)
    d2 = KGC.table_for(ct, 'direction', 2, tau, 0)[0]
    r = TK.call('ttp', np.inf, 256, 51, rays=True, groups=(2, d2))
    assert np.array_equal(r['ends'], [[0, 256], [256, 0]]) and np.array_equal(r['events'], r['casts'])
    assert_columns_sum(r)
    # source 0 (x-) emits along +x: column 1; source 1 along -x: column 0; nothing scatters, so nothing else holds a word
    assert np.array_equal(r['grp'][0, :, 1], r['sub'][0]) and np.array_equal(r['grp'][1, :, 0], r['sub'][1])
    assert not r['grp'][0, :, 0].any() and not r['grp'][1, :, 1].any() and not r['grp'][:, :, 2].any()
    assert (r['sub'][0, :, 1] >= 0).all() and (r['sub'][1, :, 1] <= 0).all() and r['sub'][0, :, 1].sum() > 0 > r['sub'][1, :, 1].sum()
    t4 = KGC.table_for(ct, 'frequency', 4, tau)[0]
    r = TK.call('ttp', np.inf, 256, 51, rays=True, groups=(4, t4))
    assert_columns_sum(r)
    unit = 2.0 ** -r['report']['k_x']
    col = KG.columns(t4, 4)
    for f in range(2):
        cm = col[r['ray_mode'][f]]
        for g in range(5):
            rays, segments = int((cm == g).sum()), int(r['ray_events'][f][cm == g].sum())
            got = float(r['grp'][f, :, g, 1].sum()) * unit
            want = (200.0 if f == 0 else -200.0) * rays
            assert allclose(got, want, rtol=0, atol=TK.TOL_TELESCOPE['ttp'] * rays + unit * segments, tag='ballistic group flux'), (f, g, got, want)
    # (the dwell words say nothing here: live modes that do not move sit for up to 38e30 ps, which sets the scale 2^k_t)
    assert (np.abs(r['grp'][:, :, :4, 1]).sum(axis=(0, 1)) > 0).all() and not r['grp'][:, :, 4].any()


@pytest.mark.parametrize('name', ['ttp_16', 'box3'])
def test_isothermal_identity_per_group(name):
    ct, tau = K.stat_inputs(name)
    p = K.STAT[name]
    t, G, _ = KGC.stat_tables(name)
    calls = [TK.call(p['case'], p['scale'], p['n'], s, groups=(G, t)) for s in p['seeds']]
    for a, b in zip(calls, TK.stat_calls(name)):            # the rays of the ungrouped statistical tests
        assert np.array_equal(a['sub'], b['sub']) and np.array_equal(a['rows'], b['rows'])
        assert_columns_sum(a)
    z, se = KGC.isothermal_deviation([r['dwell_g'] for r in calls], p['n'], ct, tau, t, G)
    print('%s: mean dT_g - 1 at most %.2f standard errors, largest standard error %.4f' % (name, z, se))
    assert z <= KGC.MAX_DEVIATION and se < KGC.MAX_SE


def test_refusals():
    """Every NK_ERR_ARG case of the grouped entry, with a text that names the cause; nothing is launched."""
    from nanokappa_amd.engine import NkError, KIN_MAX_SOURCES, KIN_MAX_GROUPS, KIN_MAX_GROUP_WORDS
    from test_gpu_free_path import fp_engine
    ct, tau, t4 = ttp_tables()
    c = K.heat_capacity(ct)
    eng = fp_engine(ct)

    def refused(text, groups, code=r'\(-2\)'):
        with pytest.raises(NkError, match=code) as e:
            eng.kinetic_flights(tau, c, n=8, groups=groups)
        assert text in str(e.value), str(e.value)

    refused('n_groups = 0 must be 1 .. 256', (0, t4))
    refused('n_groups = -3 must be 1 .. 256', (-3, t4))
    refused('n_groups = 257 must be 1 .. 256', (257, t4))
    refused('group_of_mode is NULL', (4, None))
    bad = t4.copy()
    bad[5] = 4
    refused('group_of_mode[5] = 4 is outside -1 .. 3', (4, bad))
    bad[5] = -2
    refused('group_of_mode[5] = -2 is outside -1 .. 3', (4, bad))
    refused('entries', (4, t4[:-1]), code='kinetic_flights')
    with pytest.raises(NkError, match=r'\(-2\)') as e:      # the arguments of the plain entry are refused as they are there
        eng.kinetic_flights(tau, c, n=0, groups=(4, t4))
    assert 'n_samples' in str(e.value)
    # more than 2^24 words: refused by name, but out of a caller's reach -- 8 sources x 512 subvolumes x 257 columns x 4 is less
    assert KIN_MAX_SOURCES * 512 * (KIN_MAX_GROUPS + 1) * 4 < KIN_MAX_GROUP_WORDS
    r = eng.kinetic_flights(tau, c, n=8, groups=(4, t4))
    assert r['report']['calls'] == 1 and r['grp'].shape == (2, 20, 5, 4)             # nothing ran before
    eng.close()


def test_does_not_interfere_with_the_steps():
    """test_gpu_kinetic.py's check with a grouped call (both paths of the columns) after step 10."""
    from test_gpu_replicas import assert_same_rows, assert_same_particles
    ct, tau, t4 = ttp_tables()
    pos, mode, occ, counter = random_population(ct, 30000, seed=5)
    engs, rows = [], []
    for with_call in (False, True):
        eng = make_engine(ct, pos, mode, occ, counter, seed=42)
        t0 = eng.step(10)
        if with_call:
            for bins in (True, False):
                r = eng.kinetic_flights(tau, K.heat_capacity(ct), n=500, seed=3, groups=(4, t4), lds_bins=bins)
                assert r['report']['rays'] == 1000 and r['report']['lds_bins'] == int(bins) and eng.get_step() == 10
        t1 = eng.step(10)
        engs.append(eng)
        rows.append((t0, t1))
    assert_same_rows(rows[1][0], rows[0][0], 'steps 1-10')
    assert_same_rows(rows[1][1], rows[0][1], 'steps 11-20, after the calls')
    assert_same_particles(engs[1], engs[0], 'after 20 steps')
    for e in engs:
        e.close()


def test_population_and_front_end(tmp_path):
    """--kinetic 512 --kinetic_groups 4 mfp runs through nanokappa.py and writes the two new files from 8 batches; with
    batches=2 the pooled k_kinetic.txt is summarise() of the summed integers; without groups the files are the plain call's."""
    from nanokappa_amd import nanokappa, free_path as FP
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

    with pytest.raises(ValueError, match='requires --kinetic'):
        run('refused', ['--kinetic_groups', '4', 'mfp'])
    pop = run('with', ['--kinetic', '512', '--kinetic_groups', '4', 'mfp'])
    folder = pop.results_folder_name
    for path in (KN.k_kinetic_path(folder), KN.kinetic_npz_path(folder), KG.k_kinetic_groups_path(folder), KG.kinetic_groups_npz_path(folder)):
        assert os.path.exists(path), path
    s, sg = pop.kinetic_last, pop.kinetic_groups_last
    assert s['n'] == 512 and sg['n'] == 512 and sg['batches'] == 8 and sg['G'] == 4 and sg['kind'] == 'mfp' and sg['axis'] == 0
    assert sg['grp'].shape == s['dwell'].shape + (5, 4)
    assert np.array_equal(sg['grp'][..., 0].sum(axis=2) * 2.0 ** -s['report']['k_t'], s['dwell'])
    assert np.isfinite(sg['kappa_g']).all() and np.isfinite(sg['kappa_g_se']).all() and (sg['kappa_g_se'][:4] > 0).all()
    # the flux-based and the count-based conductivity estimate the same number (the flux is conserved along the axis)
    assert abs(float(sg['kappa_flux']) - s['kappa_eff']) < 6.0 * np.hypot(float(sg['kappa_flux_se']), s['kappa_eff_se'])
    assert 0 < float(sg['kappa_flux']) < s['kappa_bulk']
    assert abs(np.nansum(sg['kappa_bulk_g']) / s['kappa_bulk'] - 1) < 1e-12
    txt, z = KG.read_k_kinetic_groups(KG.k_kinetic_groups_path(folder)), KG.read_kinetic_groups_npz(KG.kinetic_groups_npz_path(folder))
    assert txt['N'] == 512 and txt['batches'] == 8 and np.array_equal(txt['kappa_g'], sg['kappa_g'][:4]) and txt['kappa_flux'] == float(sg['kappa_flux'])
    assert np.array_equal(txt['accumulation'], np.cumsum(sg['kappa_g'][:4])) and np.array_equal(z['grp'], sg['grp'])
    # two batches: the pooled files are summarise() of the summed integers of the two engine calls under the seeds 7 and 8
    ph = pop._ph
    T = pop._mean_reservoir_T()
    tau = FP.lifetimes(ph, T)
    c = KN.heat_capacity(ph.omega, T, ph.number_of_qpoints * ph.volume_unitcell, pop.hbar, pop.kb)
    table = KG.build('mfp', 4, ph, tau, ph.group_vel)[0]
    two = pop.kinetic_flights(n=512, groups=(4, 'mfp'), batches=2)
    calls = [pop.engine.kinetic_flights(tau, c, n=256, seed=7 + b, groups=(4, table)) for b in range(2)]
    pooled = KG.pool(calls)
    assert np.array_equal(pop.kinetic_groups_last['grp'], calls[0]['grp'] + calls[1]['grp']) and pop.kinetic_groups_last['batches'] == 2
    assert np.array_equal(two['ends'], calls[0]['ends'] + calls[1]['ends']) and two['n'] == 512
    geo, src = pop._geo, KN.source_facets(pop._geo.bound_cond)
    want = KN.summarise(pooled, c, ph.group_vel, tau, T, np.asarray(geo.facets_area)[src], -np.asarray(geo.facets_normal)[src], [302.0, 298.0],
                        geo.subvol_volume, pair=KN.parallel_pair(src, geo.facets_normal, geo.facets_area, geo.facet_centroid),
                        omega_c=FP.mode_heat_capacity(np.ravel(ph.omega), T, pop.hbar, pop.kb), qv=ph.number_of_qpoints * ph.volume_unitcell)
    txt = KN.read_k_kinetic(KN.k_kinetic_path(folder))
    for k in ('G', 'G_se', 'events', 'casts'):
        assert np.array_equal(txt[k], want[k]), k
    assert txt['kappa_eff'] == want['kappa_eff'] and txt['N'] == 512
    assert KG.read_k_kinetic_groups(KG.k_kinetic_groups_path(folder))['batches'] == 2
    # a table of the caller's, one batch: no error bars
    pop.kinetic_flights(n=64, groups=(4, table), write=False)
    assert np.isnan(pop.kinetic_groups_last['kappa_g_se']).all() and pop.kinetic_groups_last['kind'] == '' and pop.current_timestep == 10
    # without groups: the plain call's bytes
    os.remove(KG.k_kinetic_groups_path(folder))
    os.remove(KG.kinetic_groups_npz_path(folder))
    pop.kinetic_flights(n=512)
    assert not os.path.exists(KG.k_kinetic_groups_path(folder)) and not os.path.exists(KG.kinetic_groups_npz_path(folder))
    with open(KN.k_kinetic_path(folder), 'rb') as f:
        mine = f.read()
    zmine = KN.read_kinetic_npz(KN.kinetic_npz_path(folder))
    pop.engine.close()
    pop = run('plain', ['--kinetic', '512'])
    with open(KN.k_kinetic_path(pop.results_folder_name), 'rb') as f:
        assert f.read() == mine
    zplain = KN.read_kinetic_npz(KN.kinetic_npz_path(pop.results_folder_name))
    assert not os.path.exists(KG.k_kinetic_groups_path(pop.results_folder_name)) and sorted(zplain) == sorted(zmine)
    for k in zplain:
        if k not in ('report_seconds', 'report_calls'):
            assert np.array_equal(zplain[k], zmine[k]), k
    pop.engine.close()
