"""Kinetic groups without a GPU: the grouped restatement (tests/kinetic_group_cases.py) against kinetic_cases.restate bit for bit,
the per-group isothermal identity with its power check, and the host side (nanokappa_amd/kinetic_groups.py): the option, the
tables, the pooling, the superposition per group and the files."""
import numpy as np
import pytest

import kinetic_cases as K
import kinetic_group_cases as KGC
import free_path_cases as FC
from nanokappa_amd import kinetic as KN
from nanokappa_amd import kinetic_groups as KG
from nanokappa_amd import field_groups as FG


@pytest.mark.parametrize('name', sorted(K.PARITY))
def test_restatement_against_restatement(name):
    """The group tally does not disturb the flights: every key of K.restate without it bit for bit, and the columns sum to sub."""
    ref, got = K.parity_run(name), KGC.parity_run(name)
    for k, v in ref.items():
        if k == 'report':
            assert got[k] == v
        else:
            assert np.array_equal(got[k], v), k
    for j in range(len(KGC.PARITY_TABLES[name])):
        grp = KGC.grp_of(got, j)
        assert grp.shape[2] == 5 and np.array_equal(grp.sum(axis=2), ref['sub'])
        assert (grp[:, :, :4, 0].sum(axis=(0, 1)) > 0).all()                      # every group flies somewhere


@pytest.mark.parametrize('name', ['ttp_16', 'box3'])
def test_isothermal_identity_per_group_and_its_power(name):
    ct, tau = K.stat_inputs(name)
    p = K.STAT[name]
    t, G, wrong = KGC.stat_tables(name)
    runs = KGC.stat_runs(name)
    for a, b in zip(runs, K.stat_runs(name)):                                     # the same flights as the ungrouped statistical tests
        assert np.array_equal(a['sub'], b['sub']) and np.array_equal(a['grp'].sum(axis=2), a['sub'])
    z, se = KGC.isothermal_deviation([r['dwell_g'] for r in runs], p['n'], ct, tau, t, G)
    print('%s: mean dT_g - 1 at most %.2f standard errors, largest standard error %.4f' % (name, z, se))
    assert z <= KGC.MAX_DEVIATION and se < KGC.MAX_SE
    # the column of mode + 1: the same check must miss
    zw, sw = KGC.isothermal_deviation([r['grp_more'][0][..., 0] * KGC.scale_t(r) for r in runs], p['n'], ct, tau, t, G)
    print('%s: with the column of mode + 1 it misses by %.1f standard errors' % (name, zw))
    assert zw > KGC.MIN_POWER


def test_option():
    assert KG.kinetic_groups_option(None) == (0, None, None) and KG.kinetic_groups_option(['0']) == (0, None, None)
    assert KG.kinetic_groups_option(['4', 'mfp'], 100) == (4, 'mfp', None)
    assert KG.kinetic_groups_option(['2', 'direction', 'y'], 100) == (2, 'direction', 1)
    assert KG.kinetic_groups_option(['3', 'branch']) == (3, 'branch', None)
    for bad in (['4'], ['x', 'mfp'], ['-1', 'mfp'], ['4', 'colour'], ['4', 'mfp', 'x'], ['4', 'direction', 'w'], ['257', 'frequency'],
                ['4', 'mfp', 'x', 'y']):
        with pytest.raises(ValueError, match='--kinetic_groups: expected G kind'):
            KG.kinetic_groups_option(bad, 100)
    with pytest.raises(ValueError, match='requires --kinetic'):
        KG.kinetic_groups_option(['4', 'mfp'], 0)
    assert KG.kinetic_groups_option([], 0) == (0, None, None)                      # off: nothing is required


def test_builders():
    ct = K.case('ttp')
    ph, v = ct['ph'], FC.group_vel(ct)
    tau = K.lifetimes(ct)
    M = v.shape[0]
    speed = np.linalg.norm(v, axis=1)
    t, G, edges = KG.build('mfp', 5, ph, tau, v)
    assert G == 5 and t.shape == (M,) and edges.shape == (6,) and t.min() == -1 and t.max() == 4
    moving = (speed > 0) & (tau > 0)
    inactive = np.asarray(getattr(ph, 'inactive_modes_mask', np.zeros(M, dtype=bool)), dtype=bool).ravel()
    assert np.array_equal(t >= 0, moving & ~inactive)                              # a mode that does not move: -1, the rest column
    # the call's own lifetimes, not the material's: other lifetimes, other bins
    tau2 = np.where(tau > 0, tau * (1.0 + 10.0 * (np.arange(M) % 7 == 0)), tau)
    t2, _, e2 = KG.build('mfp', 5, ph, tau2, v)
    ref, _, eref = FG.mfp_groups(speed * np.where(tau2 > 0, tau2, 0.0), 5, getattr(ph, 'inactive_modes_mask', None))
    assert np.array_equal(t2, ref) and np.array_equal(e2, eref) and not np.array_equal(t2, t)
    tb, _, eb = KG.build('mfp', 5, ph, K.lifetimes(ct, np.inf), v)                 # the ballistic limit's lifetimes: finite bins
    assert np.isfinite(eb).all() and tb.max() == 4
    assert np.array_equal(KG.build('frequency', 4, ph, tau, v)[0], FG.frequency_groups(ph.omega, 4, getattr(ph, 'inactive_modes_mask', None))[0])
    d, _, _ = KG.build('direction', 2, ph, tau, v, 0)
    mv = (speed > 0) & ~inactive
    assert np.array_equal(d[mv] == 1, v[mv, 0] >= 0) and (d[~mv] == -1).all()
    assert KG.build('branch', 0, ph, tau, v)[1] == ph.omega.shape[1]
    with pytest.raises(ValueError, match='unknown group kind'):
        KG.build('colour', 4, ph, tau, v)
    assert np.array_equal(KG.columns([-1, 0, 2, -1], 3), [3, 0, 2, 3])
    for G_, tab in ((0, t), (257, t), (4, None), (4, t[:-1])):
        with pytest.raises(ValueError, match='kinetic groups'):
            KG.check_table(tab, G_, M)


def _synthetic(seed=5, F=2, S=6, G=4, n=1000):
    rng = np.random.default_rng(seed)
    grp = rng.integers(-2 ** 40, 2 ** 40, (F, S, G + 1, 4))
    grp[..., 0] = np.abs(grp[..., 0])
    sub = grp.sum(axis=2)
    rep = dict(k_D=10, k_D2=3, k_T=12, k_t=20, k_x=18, n_sources=F, n_subvolumes=S, rays=F * n, events=7, casts=5, lost=0, missed=0, capped=0,
               overflow=0, seconds=0.5, calls=1)
    rows = rng.integers(0, 1000, (F, 32))
    return dict(n=n, source_facet=np.arange(F, dtype=np.int32), rows=rows, sub=sub, grp=grp, report=rep, cdf_scatter=np.ones(1), cdf_flux=np.ones(1),
                dwell=sub[..., 0] * 2.0 ** -20, flux=sub[..., 1:4] * 2.0 ** -18, dwell_g=grp[..., 0] * 2.0 ** -20, flux_g=grp[..., 1:4] * 2.0 ** -18)


def test_summary_on_synthetic_integers_and_files(tmp_path):
    ct = K.case('ttp')
    c, tau, v = K.heat_capacity(ct), K.lifetimes(ct), FC.group_vel(ct)
    src, area, n_in, cen = K.source_geometry(ct)
    pair = KN.parallel_pair(np.arange(2), -n_in, area, cen)
    ph = ct['ph']
    qv = ph.number_of_qpoints * ph.volume_unitcell
    from nanokappa_amd import free_path as FP
    omega_c = FP.mode_heat_capacity(np.ravel(ph.omega), 300.0)
    table, G, edges = KG.build('mfp', 4, ph, tau, v)
    S = len(ct['volumes'])
    batches = [_synthetic(seed=s, S=S) for s in (1, 2, 3)]
    res = KG.pool(batches)
    assert res['n'] == 3000 and res['batches'] == 3
    for k in ('rows', 'sub', 'grp'):
        assert np.array_equal(res[k], sum(b[k] for b in batches)), k
    assert np.array_equal(res['dwell_g'], res['grp'][..., 0] * 2.0 ** -20) and np.array_equal(res['flux'], res['sub'][..., 1:4] * 2.0 ** -18)
    assert np.array_equal(res['ends'], res['rows'][:, :2]) and res['report']['rays'] == 6000
    T_f = [302.0, 298.0]
    s = KG.summarise_groups(res, c, v, tau, area, n_in, T_f, ct['volumes'], table, G, pair=pair, omega_c=omega_c, qv=qv, kind='mfp', edges=edges,
                            batches=batches)
    # the groups and the rest add up to the ungrouped flux kappa, to rounding; the accumulation is the running sum
    lv = KN.live_modes(c, tau)
    g = KN.source_strength(area, n_in, c, v, lv)
    _, q = KN.profile(res, g, np.array([2.0, -2.0]), ct['volumes'], 1.0)
    want = KG.flux_kappa(q[:, 0], ct['volumes'], 200.0, 4.0, 1.0)
    assert abs(float(s['kappa_flux']) - want) <= 1e-12 * np.abs(s['kappa_g']).sum()
    assert np.array_equal(s['accumulation'], np.cumsum(s['kappa_g'][:G])) and s['kappa_g'].shape == (G + 1,)
    assert np.allclose(s['q_g'].sum(axis=1), q, rtol=1e-12, atol=1e-12 * np.abs(s['q_g']).max())
    # the per-group temperature: the c_g-weighted mean over ALL columns is kinetic.profile's dT
    dT, _ = KN.profile(res, g, np.array([2.0, -2.0]), ct['volumes'], float(np.sum(s['c_g'])))
    ok = s['c_g'] > 0
    assert np.allclose((s['dT_g'][:, ok] * s['c_g'][ok]).sum(axis=1) / s['c_g'].sum(), dT, rtol=1e-12)
    # the bulk shares add up to the bulk value, the suppression is their ratio, the error bars the spread of the batches
    tl = np.where(lv, tau, 0.0)
    assert abs(s['kappa_bulk_g'].sum() / FP.bulk_kappa(np.where(lv, omega_c, 0.0), v, tl, qv)[0, 0] - 1) < 1e-12
    assert np.allclose(s['suppression'][:G], s['kappa_g'][:G] / s['kappa_bulk_g'][:G], rtol=0, atol=0)
    per = [KG.summarise_groups(b, c, v, tau, area, n_in, T_f, ct['volumes'], table, G, pair=pair)['kappa_g'] for b in batches]
    assert np.allclose(s['kappa_g_se'], np.std(per, axis=0, ddof=1) / np.sqrt(3), rtol=1e-12)
    assert np.allclose(s['kappa_g'], np.mean(per, axis=0), rtol=1e-12)             # equal batches: the pooled value is their mean
    one = KG.summarise_groups(batches[0], c, v, tau, area, n_in, T_f, ct['volumes'], table, G, pair=pair)
    assert np.isnan(one['kappa_g_se']).all() and np.isnan(one['dT_g_se']).all() and np.isnan(one['kappa_bulk_g']).all()
    nop = KG.summarise_groups(res, c, v, tau, area, n_in, T_f, ct['volumes'], table, G)
    assert np.isnan(nop['kappa_g']).all() and nop['axis'] == -1 and np.isfinite(nop['q_g']).all()
    with pytest.raises(ValueError, match='columns'):
        KG.summarise_groups(res, c, v, tau, area, n_in, T_f, ct['volumes'], table, G + 1)
    # files
    t = KG.read_k_kinetic_groups(KG.write_k_kinetic_groups(str(tmp_path / 'k_kinetic_groups.txt'), s))
    assert t['kind'] == 'mfp' and t['N'] == 3000 and t['G'] == G and t['axis'] == 0 and t['batches'] == 3
    assert t['kappa_flux'] == float(s['kappa_flux']) and t['kappa_rest'] == s['kappa_g'][G] and t['L'] == 200.0
    for k, want in (('edge_lo', edges[:-1]), ('edge_hi', edges[1:]), ('kappa_g', s['kappa_g'][:G]), ('kappa_g_se', s['kappa_g_se'][:G]),
                    ('kappa_bulk_g', s['kappa_bulk_g'][:G]), ('suppression', s['suppression'][:G]), ('accumulation', s['accumulation'])):
        assert np.array_equal(t[k], want), k
    z = KG.read_kinetic_groups_npz(KG.write_kinetic_groups_npz(str(tmp_path / 'kinetic_groups.npz'), s))
    assert z['kind'] == 'mfp' and z['n'] == 3000 and z['G'] == G and z['batches'] == 3
    for k in ('grp', 'table', 'edges', 'dT_g', 'dT_g_se', 'q_g', 'kappa_g', 'kappa_g_se', 'accumulation', 'suppression', 'c_g'):
        assert np.array_equal(z[k], s[k], equal_nan=True), k
