"""Kinetic maps on the GPU (Engine.kinetic_flights(grid=...); nk_kinetic_flights_map, k_kinetic<GEOM, BINS, false, true>) against the
map restatement on the CPU (tests/kinetic_map_cases.py): the cells add up to the subvolumes bit for bit and everything else is the
plain call's; the same bits on every launch path; clamping into the edge cells; the launch edges; the per-cell isothermal identity
on the engine's own rays; the refusals; Population.kinetic_map and --kinetic_map.

Against the restatement a map word is held to the rule test_gpu_kinetic.py applies to `sub`: the same nonzero pattern and at most one
unit per segment (where the device logarithm's last bit rounds t the other way), so |difference| <= the call's events."""
import os
import sys

import numpy as np
import pytest

import kinetic_cases as K
import kinetic_map_cases as KMC
import free_path_cases as FC
import test_gpu_kinetic as TK
from nanokappa_amd import kinetic as KN
from nanokappa_amd import kinetic_map as KM
from util import allclose, make_engine, random_population

pytestmark = pytest.mark.gpu

PLAIN_KEYS = ('sub', 'ray_x0', 'ray_mode', 'ray_end', 'ray_events', 'ray_casts', 'ray_D', 'ray_dwell', 'ray_hash')
REPORT_KEYS = ('k_t', 'k_x', 'k_T', 'k_D', 'k_D2', 'B_t', 'B_x', 'events', 'casts', 'grid', 'geometry_mode', 'lds_bins', 'rays')
CLAMPED = KMC.ROW_CLAMPED


def plain_parity_call(name):
    p = K.PARITY[name]
    return FC.cached(('kin_map_gpu_plain', name), lambda: TK.call(p['case'], p['scale'], K.PARITY_N, p['seed'], rays=True))


def cell_sum(m):
    return m.reshape(m.shape[0], -1, 4).sum(axis=1)


def assert_map_of_plain(got, plain):
    """The exact statements: the cells sum to the subvolumes, and everything but word 25 is the plain call's."""
    assert np.array_equal(cell_sum(got['map']), got['sub'].sum(axis=1))
    assert np.array_equal(np.delete(got['rows'], CLAMPED, axis=1), np.delete(plain['rows'], CLAMPED, axis=1))
    assert np.array_equal(got['rows'][:, CLAMPED], got['clamped']) and not plain['rows'][:, CLAMPED].any()
    for k in PLAIN_KEYS:
        if k in plain:
            assert np.array_equal(got[k], plain[k]), k
    for k in REPORT_KEYS:
        assert got['report'][k] == plain['report'][k], k
    rep = got['report']
    assert np.array_equal(got['dwell_map'], got['map'][..., 0] * 2.0 ** -rep['k_t']) and np.array_equal(got['flux_map'], got['map'][..., 1:4] * 2.0 ** -rep['k_x'])


@pytest.mark.parametrize('name', ['ttp', 'ttp_16', 'ttrrp_k', 'wire72'])
def test_parity(name):
    p = K.PARITY[name]
    ct = K.case(p['case'])
    ref, plain = KMC.parity_run(name), plain_parity_call(name)
    keep = K.parity_run(name)['ray_hash'] == K.parity_run(name, fused=False)['ray_hash']
    assert keep.all()                                       # every ray is kept on the CPU: nothing is left out of the words
    for j, nc in enumerate(KMC.parity_cells(name)):
        got = TK.call(p['case'], p['scale'], K.PARITY_N, p['seed'], rays=True, grid=KMC.grid_for(ct, nc))
        assert got['report']['overflow'] == 0 and got['map'].shape == (2,) + nc + (4,)
        assert_map_of_plain(got, plain)
        assert np.array_equal(got['ray_hash'], ref['ray_hash']) and np.array_equal(got['ends'], ref['ends'])
        want, clamped = KMC.map_of(ref, j)
        events = got['report']['events']
        print('%s %r: largest |difference| of a map word %d (events %d), clamped %r' % (name, nc, np.abs(got['map'] - want).max(), events, got['clamped']))
        assert np.array_equal(got['clamped'], clamped)
        assert np.array_equal(got['map'] != 0, want != 0)
        assert allclose(got['map'], want, rtol=0, atol=events, tag='%s %r map words' % (name, nc))


def test_determinism_of_the_paths():
    p = K.PARITY['ttp_16']
    ct = K.case('ttp')
    g = KMC.grid_for(ct, (5, 3, 2))
    call = lambda **kw: TK.call('ttp', p['scale'], 300, p['seed'], rays=True, grid=g, **kw)
    plain = TK.call('ttp', p['scale'], 300, p['seed'], rays=True)
    a = call()
    assert a['report']['grid'] == 1 and a['report']['lds_bins'] == 1
    runs = [a, call(rays_per_wave=64), call(rays_per_wave=100), call(rays_per_wave=512), call(lds_bins=False), call(lds_bins=False, rays_per_wave=64), call()]
    assert runs[1]['report']['grid'] == 3 and runs[2]['report']['grid'] == 2 and runs[4]['report']['lds_bins'] == 0
    for r in runs:
        assert np.array_equal(r['map'], a['map']) and np.array_equal(r['clamped'], a['clamped'])
        assert np.array_equal(cell_sum(r['map']), r['sub'].sum(axis=1))
        for k in PLAIN_KEYS:
            assert np.array_equal(r[k], plain[k]), k
        assert np.array_equal(np.delete(r['rows'], CLAMPED, axis=1), np.delete(plain['rows'], CLAMPED, axis=1))
    # the plain call, made after the map calls: word 25 is 0 and the bits are the old ones
    after = TK.call('ttp', p['scale'], 300, p['seed'], rays=True)
    assert not after['rows'][:, CLAMPED].any() and 'map' not in after and 'clamped' not in after
    for k in PLAIN_KEYS + ('rows',):
        assert np.array_equal(after[k], plain[k]), k
    # the map of pooled batches is the elementwise integer sum of the batches' maps
    b = [TK.call('ttp', p['scale'], 300, s, grid=g) for s in (p['seed'], p['seed'] + 1)]
    pooled = KM.pool(b)
    assert np.array_equal(pooled['map'], b[0]['map'] + b[1]['map']) and np.array_equal(b[0]['map'], a['map'])
    assert np.array_equal(cell_sum(pooled['map']), pooled['sub'].sum(axis=1)) and pooled['n'] == 600


@pytest.mark.parametrize('name', ['ttp_16', 'wire72'])
def test_clamping(name):
    """A caller's grid over the middle half of the box along x: the points outside land in its edge cells and are counted."""
    p = K.PARITY[name]
    ct = K.case(p['case'])
    ref, plain = KMC.parity_run(name), plain_parity_call(name)
    got = TK.call(p['case'], p['scale'], K.PARITY_N, p['seed'], rays=True, grid=KMC.middle_half(ct, (4, 2, 2)))
    want, clamped = KMC.map_of(ref, 3)
    assert (got['clamped'] > 0).all() and np.array_equal(got['clamped'], clamped)
    assert_map_of_plain(got, plain)                         # nothing is dropped: the cells still sum to the subvolumes
    assert np.array_equal(got['map'] != 0, want != 0) and np.abs(got['map'] - want).max() <= got['report']['events']
    inner = KMC.map_of(ref, 0)[0]
    assert got['map'][:, 0, :, :, 0].sum() > got['map'][:, 1, :, :, 0].sum() and inner.shape[1] == 5       # the edge cells hold the outer quarters too


def test_launch_edges(monkeypatch):
    p = K.PARITY['ttp_16']
    ct = K.case('ttp')
    g = KMC.grid_for(ct, (5, 3, 2))
    for n, rpw in ((1, 0), (1, 1), (65, 64), (100, 7), (3, 1)):
        plain = TK.call('ttp', p['scale'], n, p['seed'], rays=True, rays_per_wave=rpw)
        got = TK.call('ttp', p['scale'], n, p['seed'], rays=True, rays_per_wave=rpw, grid=g)
        assert_map_of_plain(got, plain)
        ref = KMC.run_case('ttp', n, p['seed'], p['scale'], (KMC.key_of(g),))
        assert np.array_equal(got['map'] != 0, ref['map'] != 0) and np.abs(got['map'] - ref['map']).max() <= got['report']['events'], (n, rpw)
    # six sources on a 3 x 3 x 3 grid
    import test_gpu_kinetic_edges as TE
    six_ct = TE.E.inputs('six_sources')['ct']
    six = TE.call('six_sources', monkeypatch, grid=KMC.grid_for(six_ct, (3, 3, 3)))
    assert six['map'].shape == (6, 3, 3, 3, 4) and (six['map'][..., 0].sum(axis=(1, 2, 3)) > 0).all()
    assert_map_of_plain(six, TE.plain('six_sources', monkeypatch))
    # 64^3 cells: most stay zero, and the identity is exact
    plain = plain_parity_call('ttp')
    pp = K.PARITY['ttp']
    big = TK.call('ttp', pp['scale'], K.PARITY_N, pp['seed'], rays=True, grid=KMC.grid_for(ct, (64, 64, 64)))
    assert big['map'].shape == (2, 64, 64, 64, 4)
    assert_map_of_plain(big, plain)
    held = (big['map'] != 0).any(axis=-1).sum()
    assert 0 < held <= big['report']['events'] and held < 0.1 * 2 * 64 ** 3
    coarse = TK.call('ttp', pp['scale'], K.PARITY_N, pp['seed'], grid=KMC.grid_for(ct, (4, 4, 4)))
    assert np.array_equal(big['map'].reshape(2, 4, 16, 4, 16, 4, 16, 4).sum(axis=(2, 4, 6)), coarse['map'])      # 64 = 4 x 16: the cells nest


@pytest.mark.parametrize('name', sorted(KMC.STAT))
def test_isothermal_identity_per_cell(name):
    from nanokappa_amd.engine import cell_solid_volume
    p = KMC.STAT[name]
    ct = K.case(p['case'])
    tau = K.lifetimes(ct, p['scale'])
    lo, h, nc = KMC.stat_grid(name)
    solid = None
    if p['volume'] == 'solid':
        solid = cell_solid_volume(ct['mesh']['vertices'], ct['mesh']['faces'], lo, h, nc)
        cpu = KMC.stat_volume(name)[0]
        assert np.allclose(solid, cpu, rtol=1e-12, atol=1e-9 * float(np.prod(h)))
    V, keep = KMC.stat_volume(name, solid)
    calls = [TK.call(p['case'], p['scale'], p['n'], s, grid=(lo, h, nc)) for s in p['seeds']]
    for r in calls:
        assert np.array_equal(cell_sum(r['map']), r['sub'].sum(axis=1)) and r['report']['overflow'] == 0
    if name in K.STAT:                                      # the rays of the plain statistical tests
        for a, b in zip(calls, TK.stat_calls(name)):
            assert np.array_equal(a['sub'], b['sub']) and np.array_equal(np.delete(a['rows'], CLAMPED, axis=1), np.delete(b['rows'], CLAMPED, axis=1))
    z, se, zq = KMC.isothermal_deviation(calls, ct, tau, V, keep)
    print('%s: mean dT - 1 at most %.2f standard errors, largest standard error %.4f, q at most %.2f' % (name, z, se, zq))
    assert z <= KMC.MAX_DEVIATION and zq <= KMC.MAX_DEVIATION and se < 0.06


def test_refusals():
    """Every NK_ERR_ARG case of the map entry, with a text that names the cause; nothing is launched (the report all zero)."""
    from nanokappa_amd.engine import NkError, KIN_MAX_SOURCES, KIN_MAX_MAP_CELLS, KIN_MAX_MAP_WORDS
    from nanokappa_amd import nanokappa
    from test_gpu_free_path import fp_engine, _ttp_argv
    ct = K.case('ttp')
    tau, c = K.lifetimes(ct, 1.0 / 16.0), K.heat_capacity(ct)
    eng = fp_engine(ct)
    lo, h, nc = KMC.grid_for(ct, (4, 3, 2))

    def refused(text, grid, code=r'\(-2\)', **kw):
        with pytest.raises(NkError, match=code) as e:
            eng.kinetic_flights(tau, c, n=8, grid=grid, **kw)
        assert text in str(e.value), str(e.value)

    refused('the cell counts n must be positive', (lo, h, (4, 0, 2)))
    refused('the cell counts n must be positive', (lo, h, (-1, 3, 2)))
    refused('the cell sizes h must be positive and finite', (lo, [h[0], 0.0, h[2]], nc))
    refused('the cell sizes h must be positive and finite', (lo, [h[0], -1.0, h[2]], nc))
    refused('the cell sizes h must be positive and finite', (lo, [np.inf, h[1], h[2]], nc))
    refused('the cell sizes h must be positive and finite', (lo, [h[0], h[1], np.nan], nc))
    refused('the corner lo must be finite', ([np.nan, 0.0, 0.0], h, nc))
    refused('the corner lo must be finite', ([0.0, -np.inf, 0.0], h, nc))
    refused('16777217 cells are more than the grid takes (2^24)', (lo, h, (16777217, 1, 1)))
    refused('16781312 cells are more than the grid takes (2^24)', (lo, h, (4097, 4096, 1)))
    assert 2 * KIN_MAX_MAP_CELLS * 4 <= KIN_MAX_MAP_WORDS < KIN_MAX_SOURCES * KIN_MAX_MAP_CELLS * 4        # (two sources never reach the word bound)
    refused('grid must be (lo [3], h [3], n_cells [3])', (lo, h, (4, 3)), code='kinetic_flights')
    refused('grid and groups were both given', (lo, h, nc), code='kinetic_flights', groups=(1, np.zeros(tau.shape[0], dtype=np.int32)))
    with pytest.raises(NkError, match=r'\(-2\)') as e:      # the arguments of the plain entry are refused as they are there, in its words
        eng.kinetic_flights(tau, c, n=0, grid=(lo, h, nc))
    assert 'nk_kinetic_flights: n_samples = 0 must be positive' in str(e.value)
    # a NULL grid, and the report of a refused call: straight at the C entry
    import ctypes as C
    from nanokappa_amd import engine as EN
    a, o, rep = EN.nk_kinetic_args(), EN.nk_kinetic_out(), EN.nk_kinetic_report()
    cs, cf = KN.tables(c, tau, FC.group_vel(ct))
    t_ = np.ascontiguousarray(tau)
    a.n_samples, a.tau, a.cdf_scatter, a.cdf_flux = 8, EN._p(t_), EN._p(cs), EN._p(cf)
    rep.calls = 77
    assert eng.L.nk_kinetic_flights_map(eng.h, C.byref(a), None, C.byref(o), None, None, C.byref(rep)) == EN.ERR_ARG
    assert 'grid is NULL' in eng.L.nk_last_error(eng.h).decode() and bytes(rep) == bytes(EN.nk_kinetic_report())
    bad = EN.nk_kinetic_grid()
    bad.n[:], bad.lo[:], bad.h[:] = [2048, 2048, 2048], list(lo), list(h)
    rep.calls = 77
    assert eng.L.nk_kinetic_flights_map(eng.h, C.byref(a), C.byref(bad), C.byref(o), None, None, C.byref(rep)) == EN.ERR_ARG
    assert 'cells are more than the grid takes' in eng.L.nk_last_error(eng.h).decode() and bytes(rep) == bytes(EN.nk_kinetic_report())
    r = eng.kinetic_flights(tau, c, n=8, grid=(lo, h, nc))
    assert r['report']['calls'] == 1 and r['map'].shape == (2, 4, 3, 2, 4)          # nothing ran before
    eng.close()
    # the front end: --kinetic_map without --kinetic, before anything is set up
    with pytest.raises(ValueError, match='--kinetic_map requires --kinetic N'):
        nanokappa.main(_ttp_argv(2000, 10, ['--kinetic_map', '4', '3', '2']))


def test_word_bound_with_six_sources(monkeypatch):
    """n_sources * ncells * 4 above 2^27 words: six sources on 2^23 cells are refused by name, two sources are not the limit."""
    from nanokappa_amd.engine import NkError
    import test_gpu_kinetic_edges as TE
    six_ct = TE.E.inputs('six_sources')['ct']
    lo, h, _ = KMC.grid_for(six_ct, (1, 1, 1))
    with pytest.raises(NkError, match=r'\(-2\)') as e:
        TE.call('six_sources', monkeypatch, grid=(lo, h / 256.0, (256, 256, 128)))
    assert '6 sources x 8388608 cells x 4 = 201326592 words are more than a call takes (2^27)' in str(e.value)


def test_does_not_interfere_with_the_steps():
    """test_gpu_kinetic.py's check with map calls (both paths of the subvolume words) after step 10."""
    from test_gpu_replicas import assert_same_rows, assert_same_particles
    ct = K.case('ttp')
    tau = K.lifetimes(ct, 1.0 / 16.0)
    g = KMC.grid_for(ct, (5, 3, 2))
    pos, mode, occ, counter = random_population(ct, 30000, seed=5)
    engs, rows = [], []
    for with_call in (False, True):
        eng = make_engine(ct, pos, mode, occ, counter, seed=42)
        t0 = eng.step(10)
        if with_call:
            for bins in (True, False):
                r = eng.kinetic_flights(tau, K.heat_capacity(ct), n=500, seed=3, grid=g, lds_bins=bins)
                assert r['report']['rays'] == 1000 and r['report']['lds_bins'] == int(bins) and eng.get_step() == 10
                assert np.array_equal(cell_sum(r['map']), r['sub'].sum(axis=1))
        t1 = eng.step(10)
        engs.append(eng)
        rows.append((t0, t1))
    assert_same_rows(rows[1][0], rows[0][0], 'steps 1-10')
    assert_same_rows(rows[1][1], rows[0][1], 'steps 11-20, after the calls')
    assert_same_particles(engs[1], engs[0], 'after 20 steps')
    for e in engs:
        e.close()


def test_population_and_front_end(tmp_path):
    """--kinetic 512 --kinetic_map 5 3 2 solid runs through nanokappa.py and writes the two map files from 8 batches beside
    k_kinetic.txt and kinetic.npz of the pooled batches; with --kinetic_groups as well the grouped flights write those two and the
    files agree; without the option the set of files and their bytes are the plain call's."""
    from nanokappa_amd import nanokappa
    from nanokappa_amd import kinetic_groups as KG
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
        run('refused', ['--kinetic_map', '5', '3', '2'])
    pop = run('with', ['--kinetic', '512', '--kinetic_map', '5', '3', '2', 'solid'])
    folder = pop.results_folder_name
    for path in (KN.k_kinetic_path(folder), KN.kinetic_npz_path(folder), KM.kinetic_map_npz_path(folder), KM.kinetic_map_vtk_path(folder)):
        assert os.path.exists(path), path
    assert not os.path.exists(KG.k_kinetic_groups_path(folder))
    s, m = pop.kinetic_last, pop.kinetic_map_last
    assert s['n'] == 512 and m['n_samples'] == 512 and m['batches'] == 8 and m['n'] == (5, 3, 2) and m['volume'] == 'solid'
    assert m['T'].shape == (5, 3, 2) and m['q'].shape == (5, 3, 2, 3) and np.isfinite(m['T']).all() and np.isfinite(m['q']).all()
    assert np.isfinite(m['T_se']).all() and (m['T_se'] > 0).all() and np.isfinite(m['q_se']).all()
    assert np.allclose(m['solid_fraction'], 1.0, rtol=0, atol=1e-12) and pop.current_timestep == 10
    assert np.array_equal(m['map'][..., 0].sum(axis=(1, 2, 3)) * 2.0 ** -s['report']['k_t'], s['dwell'].sum(axis=1))
    assert m['q'][..., 0].mean() > 0 and m['T_ref'] == 300.0                                    # 302 K at x-, 298 K at x+: heat flows along +x
    z, v = KM.read_kinetic_map_npz(KM.kinetic_map_npz_path(folder)), KM.read_kinetic_map_vtk(KM.kinetic_map_vtk_path(folder))
    for k in ('T', 'dT', 'T_se', 'q', 'q_se', 'map', 'solid_fraction'):
        assert np.array_equal(z[k], m[k]), k
    for k in ('T', 'dT', 'T_se', 'dT_se', 'q', 'q_se', 'solid_fraction'):
        assert np.array_equal(v[k], m[k]), k
    assert v['n'] == (5, 3, 2) and '%d points clamped' % m['clamped'].sum() in v['title'] and z['batches'] == 8
    # k_kinetic.txt is summarise() of the pooled integers of the 8 engine calls under the seeds 7 .. 14
    from nanokappa_amd import free_path as FP
    from nanokappa_amd import field as FD
    ph = pop._ph
    T = pop._mean_reservoir_T()
    tau = FP.lifetimes(ph, T)
    c = KN.heat_capacity(ph.omega, T, ph.number_of_qpoints * ph.volume_unitcell, pop.hbar, pop.kb)
    grid = FD.grid_from_bounds(pop._geo.bounds, (5, 3, 2))
    calls = [pop.engine.kinetic_flights(tau, c, n=64, seed=7 + b, grid=grid) for b in range(8)]
    assert np.array_equal(m['map'], sum(r['map'] for r in calls))
    txt = KN.read_k_kinetic(KN.k_kinetic_path(folder))
    assert txt['N'] == 512 and np.array_equal(txt['events'], sum(r['events'] for r in calls)) and np.array_equal(txt['G'], s['G'])
    # Population.kinetic_map: cell volume, one batch: no error bars; nothing is written with write=False
    os.remove(KM.kinetic_map_npz_path(folder))
    one = pop.kinetic_map((3, 1, 1), n=64, batches=1, write=False)
    assert np.isnan(one['T_se']).all() and np.isfinite(one['T']).all() and 'solid_fraction' not in one and not os.path.exists(KM.kinetic_map_npz_path(folder))
    pop.engine.close()
    # with groups as well: the grouped flights write k_kinetic.txt, the mapped ones the map; rows and sub are the same bits
    pop = run('both', ['--kinetic', '512', '--kinetic_groups', '4', 'mfp', '--kinetic_map', '5', '3', '2'])
    both = pop.results_folder_name
    for path in (KN.k_kinetic_path(both), KG.k_kinetic_groups_path(both), KM.kinetic_map_npz_path(both), KM.kinetic_map_vtk_path(both)):
        assert os.path.exists(path), path
    assert np.array_equal(pop.kinetic_map_last['map'], m['map']) and pop.kinetic_map_last['volume'] == 'cell'
    assert np.array_equal(pop.kinetic_groups_last['grp'].sum(axis=2), KM.pool(calls)['sub'])
    with open(KN.k_kinetic_path(both), 'rb') as f, open(KN.k_kinetic_path(folder), 'rb') as g:
        assert f.read() == g.read()
    pop.engine.close()
    # without the option: the plain call's files, byte for byte what Population.kinetic_flights writes
    pop = run('plain', ['--kinetic', '512'])
    plain = pop.results_folder_name
    assert not os.path.exists(KM.kinetic_map_npz_path(plain)) and not os.path.exists(KM.kinetic_map_vtk_path(plain))
    with open(KN.k_kinetic_path(plain), 'rb') as f:
        first = f.read()
    zfirst = KN.read_kinetic_npz(KN.kinetic_npz_path(plain))
    names = sorted(os.listdir(plain))
    pop.kinetic_flights(n=512)
    with open(KN.k_kinetic_path(plain), 'rb') as f:
        assert f.read() == first
    zagain = KN.read_kinetic_npz(KN.kinetic_npz_path(plain))
    assert sorted(os.listdir(plain)) == names and sorted(zagain) == sorted(zfirst)
    for k in zfirst:
        if k not in ('report_seconds', 'report_calls'):
            assert np.array_equal(zfirst[k], zagain[k]), k
    want = pop.engine.kinetic_flights(tau, c, n=512)                     # one plain engine call under the run's seed: the option's absence changes nothing
    assert np.array_equal(zfirst['ends'], want['ends']) and np.array_equal(zfirst['dwell'], want['dwell'])
    pop.engine.close()
