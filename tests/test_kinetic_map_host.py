"""Kinetic maps without a GPU: the map restatement (tests/kinetic_map_cases.py) against kinetic_cases.restate bit for bit, the
cell-sum identity, the per-cell isothermal identity with its power check, and the host side (nanokappa_amd/kinetic_map.py): the
option, the pooling, summarise_map with its volumes, NaN rules and standard errors, and the files."""
import numpy as np
import pytest

import kinetic_cases as K
import kinetic_map_cases as KMC
import free_path_cases as FC
from nanokappa_amd import field as FD
from nanokappa_amd import kinetic as KN
from nanokappa_amd import kinetic_map as KM


def cell_sum(m):
    """The sum of a map [F, nx, ny, nz, 4] over its cells: [F, 4]."""
    return m.reshape(m.shape[0], -1, 4).sum(axis=1)


@pytest.mark.parametrize('name', sorted(K.PARITY))
def test_restatement_against_restatement(name):
    """The map tally does not disturb the flights: every key of K.restate without it bit for bit (rows but for word 25), and the
    cells sum to the subvolumes."""
    ref, got = K.parity_run(name), KMC.parity_run(name)
    for k, v in ref.items():
        if k == 'report':
            assert got[k] == v
        elif k == 'rows':
            assert np.array_equal(np.delete(got[k], KMC.ROW_CLAMPED, axis=1), np.delete(v, KMC.ROW_CLAMPED, axis=1))
            assert not v[:, KMC.ROW_CLAMPED].any() and np.array_equal(got[k][:, KMC.ROW_CLAMPED], got['clamped'])
        else:
            assert np.array_equal(got[k], v), k
    cells = KMC.parity_cells(name) + ((4, 2, 2),)
    for j, nc in enumerate(cells):
        m, cl = KMC.map_of(got, j)
        assert m.shape == (2,) + nc + (4,)
        assert np.array_equal(cell_sum(m), ref['sub'].sum(axis=1)), nc            # for every source and word, exactly
        # over the bounds next to nothing is clamped; the grid over the middle half clamps the outer quarters into its edge cells
        assert (cl > 0).all() if j == 3 else (cl <= 2).all()
    one = KMC.map_of(got, 1)[0]
    assert np.array_equal(one[:, 0, 0, 0], ref['sub'].sum(axis=1))
    assert np.array_equal(got['dwell_map'], got['map'][..., 0] * 2.0 ** -got['report']['k_t'])
    assert np.array_equal(got['flux_map'], got['map'][..., 1:4] * 2.0 ** -got['report']['k_x'])


def test_slices_are_cells_on_ttp():
    """'ttp' is cut into 20 slices of 10 A along x, and 10 is a double: with n = (20, 1, 1) over the bounds the floor rule and the
    slice classifier agree on every segment point of this seed, so the map IS sub."""
    p = K.PARITY['ttp']
    ct = K.case('ttp')
    S = int(K.subvols(ct).S)
    r = KMC.run_case('ttp', K.PARITY_N, p['seed'], p['scale'], (KMC.key_of(KMC.grid_for(ct, (S, 1, 1))),))
    assert r['map'].shape == (2, S, 1, 1, 4) and np.array_equal(r['map'][:, :, 0, 0], r['sub']) and not r['clamped'].any()


@pytest.mark.parametrize('name', sorted(KMC.STAT))
def test_isothermal_identity_per_cell_and_its_power(name):
    p = KMC.STAT[name]
    ct = K.case(p['case'])
    tau = K.lifetimes(ct, p['scale'])
    runs = KMC.stat_runs(name)
    V, keep = KMC.stat_volume(name)                         # (asserts the cap on the cells left out)
    assert max(p['cells']) <= 4 and keep.sum() >= 0.75 * (V > 0).sum()
    for r in runs:
        assert np.array_equal(cell_sum(r['map']), r['sub'].sum(axis=1)) and np.array_equal(cell_sum(r['map_more'][0][0]), r['sub'].sum(axis=1))
    if name in K.STAT:                                      # the same flights as the plain statistical tests
        for a, b in zip(runs, K.stat_runs(name)):
            assert np.array_equal(a['sub'], b['sub'])
    z, se, zq = KMC.isothermal_deviation(runs, ct, tau, V, keep)
    print('%s: mean dT - 1 at most %.2f standard errors, largest standard error %.4f, q at most %.2f' % (name, z, se, zq))
    assert z <= KMC.MAX_DEVIATION and zq <= KMC.MAX_DEVIATION and se < 0.06
    # the start point instead of x_p: the same check must miss
    wrong = [KMC.as_result(r['n'], r['map_more'][0][0][..., 0] * 2.0 ** -r['report']['k_t'], r['map_more'][0][0][..., 1:4] * 2.0 ** -r['report']['k_x'])
             for r in runs]
    zw, _, zqw = KMC.isothermal_deviation(wrong, ct, tau, V, keep)
    print('%s: binned by the start point it misses by %.1f (dT) and %.1f (q) standard errors' % (name, zw, zqw))
    assert max(zw, zqw) > KMC.MIN_POWER


def test_option():
    assert KM.kinetic_map_option(None) == (None, 'cell') and KM.kinetic_map_option([]) == (None, 'cell')
    assert KM.kinetic_map_option(['0', '0', '0']) == (None, 'cell') and KM.kinetic_map_option(['0', '0', '0', 'solid']) == (None, 'solid')
    assert KM.kinetic_map_option(['4', '3', '2'], 100) == ((4, 3, 2), 'cell')
    assert KM.kinetic_map_option(['4', '3', '2', 'solid'], 100) == ((4, 3, 2), 'solid')
    assert KM.kinetic_map_option(['256', '256', '256', 'cell']) == ((256, 256, 256), 'cell')
    for bad in (['4'], ['4', '3'], ['4', '3', 'x'], ['4', '3', '2', 'count'], ['4', '3', '2', 'solid', '1'], ['4', '0', '2'], ['-1', '3', '2'],
                ['257', '256', '256']):
        with pytest.raises(ValueError, match=r'--kinetic_map: expected nx ny nz \[cell\|solid\]') as e:
            KM.kinetic_map_option(bad, 100)
        assert repr(' '.join(bad)) in str(e.value)
    with pytest.raises(ValueError, match='--kinetic_map requires --kinetic N'):
        KM.kinetic_map_option(['4', '3', '2'], 0)
    assert KM.kinetic_map_option([], 0) == (None, 'cell')                          # off: nothing is required


def test_pool_is_additive():
    p = K.PARITY['ttp_16']
    ct = K.case('ttp')
    g = KMC.key_of(KMC.grid_for(ct, (5, 3, 2)))
    a, b = (KMC.run_case('ttp', 64, s, p['scale'], (g,)) for s in (5, 6))
    for r in (a, b):
        r['report'].setdefault('message', '')
    pooled = KM.pool([a, b])
    for k in ('rows', 'sub', 'map', 'clamped'):
        assert np.array_equal(pooled[k], a[k] + b[k]), k
    assert pooled['n'] == 128 and pooled['batches'] == 2
    assert np.array_equal(pooled['dwell_map'], pooled['map'][..., 0] * 2.0 ** -a['report']['k_t'])
    assert np.array_equal(cell_sum(pooled['map']), pooled['sub'].sum(axis=1))
    other = KMC.run_case('ttp', 64, 5, p['scale'], (KMC.key_of(KMC.grid_for(ct, (1, 1, 1))),))
    other['report'].setdefault('message', '')
    with pytest.raises(ValueError, match='differ in their grid'):
        KM.pool([a, other])


def _inputs(nc=(3, 2, 2), seeds=(5, 6, 7)):
    p = K.PARITY['ttp_16']
    ct = K.case('ttp')
    lo, h, nc = KMC.grid_for(ct, nc)
    runs = [KMC.run_case('ttp', 64, s, p['scale'], (KMC.key_of((lo, h, nc)),)) for s in seeds]
    for r in runs:
        r['report'].setdefault('message', '')
    c, tau = K.heat_capacity(ct), K.lifetimes(ct, p['scale'])
    src, area, n_in, _ = K.source_geometry(ct)
    return ct, runs, c, tau, area, n_in, (lo, h, nc)


def test_summarise_map():
    ct, runs, c, tau, area, n_in, (lo, h, nc) = _inputs()
    v = FC.group_vel(ct)
    pooled = KM.pool(runs)
    s = KM.summarise_map(pooled, c, v, tau, area, n_in, [302.0, 298.0], lo, h, nc, batches=runs)
    assert s['n'] == nc and s['batches'] == 3 and s['T_ref'] == 300.0 and s['volume'] == 'cell' and 'solid_fraction' not in s
    assert s['T'].shape == nc and s['q'].shape == nc + (3,) and np.array_equal(s['T'], 300.0 + s['dT']) and np.array_equal(s['T_se'], s['dT_se'])
    assert np.isfinite(s['T']).all() and np.isfinite(s['T_se']).all() and (s['T_se'] > 0).all() and np.isfinite(s['q_se']).all()
    assert np.array_equal(s['cell_volume'], np.full(nc, np.prod(h)))
    # one formula: kinetic.profile on the cells
    lv = KN.live_modes(c, tau)
    g = KN.source_strength(area, n_in, c, v, lv)
    import math
    dT, q = KN.profile(dict(n=pooled['n'], dwell=pooled['dwell_map'].reshape(2, -1), flux=pooled['flux_map'].reshape(2, -1, 3)), g,
                       np.array([2.0, -2.0]), np.full(12, np.prod(h)), math.fsum(c[lv]))
    assert np.array_equal(s['dT'], dT.reshape(nc)) and np.array_equal(s['q'], q.reshape(nc + (3,)))
    assert s['dT'][0].mean() > 0 > s['dT'][-1].mean() and s['q'][..., 0].mean() > 0        # hot at x-, heat flows along +x
    # the standard error: std(ddof = 1) / sqrt(B) of the batches' own cell quantities
    per = np.array([KM.summarise_map(r, c, v, tau, area, n_in, [302.0, 298.0], lo, h, nc)['dT'] for r in runs])
    assert np.allclose(s['dT_se'], per.std(axis=0, ddof=1) / np.sqrt(3), rtol=1e-13, atol=0)
    one = KM.summarise_map(runs[0], c, v, tau, area, n_in, [302.0, 298.0], lo, h, nc)
    assert one['batches'] == 1 and np.isnan(one['dT_se']).all() and np.isnan(one['q_se']).all() and np.isfinite(one['dT']).all()
    assert np.isnan(KM.summarise_map(runs[0], c, v, tau, area, n_in, [302.0, 298.0], lo, h, nc, batches=runs[:1])['T_se']).all()
    # solid: the volumes of the caller, the fraction, NaN where there is no solid and where nothing dwelt
    V = np.full(nc, np.prod(h))
    V[0, 0, 0] *= 0.5
    V[2, 1, 1] = 0.0
    sol = KM.summarise_map(pooled, c, v, tau, area, n_in, [302.0, 298.0], lo, h, nc, volume='solid', solid_volume=V, batches=runs)
    assert np.array_equal(sol['solid_fraction'], V / np.prod(h)) and sol['solid_fraction'][0, 0, 0] == 0.5
    assert np.isnan(sol['T'][2, 1, 1]) and np.isnan(sol['q'][2, 1, 1]).all() and np.isnan(sol['T_se'][2, 1, 1])
    assert np.allclose(sol['dT'][0, 0, 0], 2.0 * s['dT'][0, 0, 0], rtol=1e-15) and np.isnan(sol['T']).sum() == 1
    rest = np.ones(nc, dtype=bool)
    rest[0, 0, 0] = rest[2, 1, 1] = False
    assert np.array_equal(sol['dT'][rest], s['dT'][rest])
    empty = dict(pooled, map=pooled['map'].copy())
    empty['map'][:, 1, 0, 1] = 0
    empty.update(dwell_map=empty['map'][..., 0] * 2.0 ** -pooled['report']['k_t'], flux_map=empty['map'][..., 1:4] * 2.0 ** -pooled['report']['k_x'])
    e = KM.summarise_map(empty, c, v, tau, area, n_in, [302.0, 298.0], lo, h, nc)
    assert np.isnan(e['T'][1, 0, 1]) and np.isnan(e['q'][1, 0, 1]).all() and np.isnan(e['T']).sum() == 1       # NaN, not T_ref
    with pytest.raises(ValueError, match="volume must be one of cell, solid"):
        KM.summarise_map(pooled, c, v, tau, area, n_in, [302.0, 298.0], lo, h, nc, volume='count')
    with pytest.raises(ValueError, match="needs solid_volume"):
        KM.summarise_map(pooled, c, v, tau, area, n_in, [302.0, 298.0], lo, h, nc, volume='solid')
    with pytest.raises(ValueError, match='the map has the shape'):
        KM.summarise_map(pooled, c, v, tau, area, n_in, [302.0, 298.0], lo, h, (2, 2, 3))


def test_isothermal_input_gives_one_kelvin():
    """A map whose dwell is what an isothermal solid 1 K above the reference holds -- per source g_f N V_c c_total / sum g of
    dwell in a cell of volume V_c -- gives dT = 1 K in every cell, with the cell and with the solid volumes."""
    import math
    ct, runs, c, tau, area, n_in, (lo, h, nc) = _inputs()
    lv = KN.live_modes(c, tau)
    g = KN.source_strength(area, n_in, c, FC.group_vel(ct), lv)
    ctot = math.fsum(c[lv])
    V = np.full(nc, np.prod(h))
    V[1, 1, 0] *= 0.25
    N = 1000
    for vol, kw in ((np.full(nc, np.prod(h)), {}), (V, dict(volume='solid', solid_volume=V))):
        dwell = np.stack([np.full(nc, N * ctot * KN.watt() / g.sum()) * vol for _ in range(2)])
        res = dict(n=N, dwell_map=dwell, flux_map=np.zeros((2,) + nc + (3,)), map=np.ones((2,) + nc + (4,), dtype=np.int64), clamped=np.zeros(2, dtype=np.int64),
                   source_facet=np.arange(2), report={})
        s = KM.summarise_map(res, c, FC.group_vel(ct), tau, area, n_in, [301.0, 301.0], lo, h, nc, **kw)
        assert s['T_ref'] == 301.0 and np.array_equal(s['dT'], np.zeros(nc))      # the superposition around the mean: nothing deviates
        dT, q = KM.cell_profile(res, g, np.ones(2), vol, ctot)
        assert np.allclose(dT, 1.0, rtol=1e-14, atol=0) and not q.any()


def test_files_round_trip(tmp_path):
    ct, runs, c, tau, area, n_in, (lo, h, nc) = _inputs()
    pooled = KM.pool(runs)
    V = np.full(nc, np.prod(h))
    V[0, 1, 0] *= 0.5
    for kw in ({}, dict(volume='solid', solid_volume=V)):
        s = KM.summarise_map(pooled, c, FC.group_vel(ct), tau, area, n_in, [302.0, 298.0], lo, h, nc, batches=runs, **kw)
        s['clamped'] = np.array([3, 4])
        z = KM.read_kinetic_map_npz(KM.write_kinetic_map_npz(KM.kinetic_map_npz_path(str(tmp_path)), s))
        for k in ('dT', 'dT_se', 'T', 'T_se', 'q', 'q_se', 'map', 'clamped', 'cell_volume', 'lo', 'h', 'g', 'T_f'):
            assert np.array_equal(z[k], s[k], equal_nan=True), k
        assert z['n'] == nc and z['volume'] == s['volume'] and z['batches'] == 3 and z['n_samples'] == 192 and z['T_ref'] == 300.0
        assert z['report']['k_t'] == pooled['report']['k_t'] and ('solid_fraction' in z) == bool(kw)
        v = KM.read_kinetic_map_vtk(KM.write_kinetic_map_vtk(KM.kinetic_map_vtk_path(str(tmp_path)), s))
        assert v['n'] == nc and np.array_equal(v['lo'], lo) and np.array_equal(v['h'], h) and '7 points clamped' in v['title']
        for k in ('T', 'dT', 'T_se', 'dT_se', 'q', 'q_se'):
            assert np.array_equal(v[k], s[k], equal_nan=True), k
        assert ('solid_fraction' in v) == bool(kw)
        if kw:
            assert np.array_equal(v['solid_fraction'], V / np.prod(h)) and np.array_equal(z['solid_fraction'], V / np.prod(h))
    # the layout is field.vtk's: the same reader, the same cell order
    assert FD.read_vtk(KM.kinetic_map_vtk_path(str(tmp_path)))['T'].shape == nc
