"""Grouped field maps on the GPU (nk_set_field_groups / k_field<., true>): the sums over the groups against the field's own
integers, state mode against the host restatement, step mode against the oracle's particles, a slab grid against the band rows
of k_spectral, the two paths, a store that regrows in mid-window, degenerate shapes, errors and lifetime, a one-rank
communicator and the Population outputs (field_groups.npz)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from util import (case_tables, random_population, make_oracle_sim, make_engine, same_event_rule, rel_row, TOL_ROW_ERAW,
                  TOL_ROW_FLUX, TOL_RUN_ERAW, TOL_T)
from test_gpu_field import state_on_host, quant_bound, check_against_row, TOL_FIELD_STATE

pytestmark = pytest.mark.gpu

GRID = (5, 3, 2)                    # sizes that are neither one nor powers of two


def grid_of(ct, n=GRID):
    from nanokappa_amd import field as FD
    return FD.grid_from_bounds(ct['mesh']['bounds'], n)


def table_all(M, G=4):
    """Every mode in a group: mode % G."""
    return (np.arange(M) % G).astype(np.int32), G


def table_some(M):
    """G = 3: mode % 4, the value 3 mapped to -1 -- a quarter of the modes is in no group."""
    g = (np.arange(M) % 4).astype(np.int32)
    g[g == 3] = -1
    return g, 3


def engine_with_groups(ct, pop4, table, G, n=GRID, seed=3, every=10, flags=0, **kw):
    pos, mode, occ, counter = pop4
    eng = make_engine(ct, pos, mode, occ, counter, seed=seed, **kw)
    lo, h, n = grid_of(ct, n)
    eng.set_field(lo, h, n, every, flags=flags)
    eng.set_field_groups(table, G)
    return eng, (lo, h, n)


def assert_groups_add_up_to_field(eng, label=''):
    """State mode: the integers summed over the groups are the field's integers (every mode grouped)."""
    sf = eng.tally_field_state()
    sg = eng.tally_field_groups_state()
    assert sg['raw'].dtype == np.int64 and sg['raw'].shape == sf['raw'].shape[:3] + (sg['raw'].shape[3], 8)
    assert np.array_equal(sg['raw'].sum(axis=3)[..., :5], sf['raw'][..., :5]), 'state integers ' + label
    assert not sg['raw'][..., 5:].any()
    assert sg['clamped'] == sf['clamped'] and sg['ungrouped'] == 0
    assert (sg['k_E'], sg['k_F']) == (sf['k_E'], sf['k_F'])
    return sf, sg


def assert_windows_add_up(f, g, label=''):
    """Step mode: the accumulated doubles summed over the groups equal the field's accumulated doubles (multiples of 2^-k
    far below 2^53 units: every addition is exact)."""
    assert g['samples'] == f['samples'] and g['ungrouped'] == 0
    assert np.array_equal(g['N'].sum(axis=3), f['N']), 'N ' + label
    assert np.array_equal(g['E'].sum(axis=3), f['E']), 'E ' + label
    assert np.array_equal(g['F'].sum(axis=3), f['F']), 'F ' + label


# ---------------------------------------------------------------------------------------------- 1. groups add up to the field
@pytest.mark.parametrize('case,nobox', [('ttp', False), ('ttp', True), ('ttrrp', False)])
def test_groups_add_up_to_the_field(case, nobox, monkeypatch):
    if nobox:
        monkeypatch.setenv('NK_NO_BOX', '1')
    ct = case_tables(case)
    pop4 = random_population(ct, 20000, seed=5, T0=303.0)
    table, G = table_all(ct['M'])
    eng, _ = engine_with_groups(ct, pop4, table, G)
    if nobox:
        assert int(eng.timing()['box_store']) == 0
    info = eng.field_groups_info()
    assert info['on'] == 1 and info['G'] == 4 and info['lines'] == 5 * 3 * 2 * 4 and info['bytes'] > 0 and info['lds_path'] == 1
    assert_groups_add_up_to_field(eng, 'before the first step')
    eng.step(20)
    f, g = eng.field(), eng.field_groups()
    assert f['samples'] == 2
    assert_windows_add_up(f, g)
    assert g['N'].sum() == f['N'].sum() > 0 and np.abs(g['E']).max() > 0 and np.abs(g['F']).max() > 0
    assert np.count_nonzero(g['N'].sum(axis=(0, 1, 2))) == 4                # every group holds particles
    assert_groups_add_up_to_field(eng, 'after 20 steps')


# ---------------------------------------------------------------------------------------------- 2. state mode against the host
@pytest.mark.parametrize('case', ['ttp', 'ttrrp'])
def test_state_mode_against_host(case):
    from nanokappa_amd import field_groups as FG
    ct = case_tables(case)
    pop4 = random_population(ct, 20000, seed=12, T0=303.0)                  # 5 K above the subvolumes: e_i of full size
    table, G = table_some(ct['M'])
    eng, (lo, h, n) = engine_with_groups(ct, pop4, table, G, seed=2)
    eng.step(7)
    st = eng.tally_field_groups_state()
    x, e, v = state_on_host(eng, ct)
    grp = table[eng.download()['mode'].astype(int)]
    ref = FG.groups_from_particles(x, e, v, grp, lo, h, n, G)
    q = FG.quantised(x, e, v, grp, lo, h, n, G, st['k_E'], st['k_F'])
    assert st['ungrouped'] == int((grp < 0).sum()) == ref['ungrouped'] > 0
    assert np.array_equal(st['N'], ref['N']) and np.array_equal(st['raw'][..., 0], q['raw'][..., 0])
    assert st['N'].sum() + st['ungrouped'] == x.shape[0] == eng.timing()['live']
    assert st['clamped'] == ref['clamped']
    for key, k in (('E', st['k_E']), ('F', st['k_F'])):
        nb = ref['N'] if key == 'E' else ref['N'][..., None]
        term = np.max(np.abs(e)) if key == 'E' else np.max(np.abs(v * e[:, None]))
        dev = np.abs(st[key] - ref[key]) - quant_bound(nb, k) - nb * np.ldexp(term, -53)
        worst = float(np.max(dev) / np.max(np.abs(ref[key])))
        rel_row(st[key], ref[key], tag='field groups state ' + key)
        print('state mode %s: deviation less the rounding bound: %.3e of the largest line' % (key, worst))
        assert worst <= TOL_FIELD_STATE
    # the device's integers against the host's integers of the host's terms (the field's TOL_FIELD_STATE = 0: equal)
    for key, sl, k in (('E', slice(1, 2), st['k_E']), ('F', slice(2, 5), st['k_F'])):
        du = np.max(np.abs(st['raw'][..., sl] - q['raw'][..., sl]))
        print('state mode %s: device integers against host integers: %d units' % (key, du))
        assert float(np.ldexp(float(du), -k) / np.max(np.abs(ref[key]))) <= TOL_FIELD_STATE


# ---------------------------------------------------------------------------------------------- 3. step mode against the oracle
def oracle_sample(sim, table, G, grid):
    from nanokappa_amd import field_groups as FG
    lo, h, n = grid
    P = sim.P
    k = P.N
    m = P.mode[:k].astype(int)
    vg = sim.mat.group_vel_array.reshape(-1, 3)
    return FG.groups_from_particles(P.pos[:k], P.energy[:k], vg[m], table[m], lo, h, n, G)


def check_window_against_oracle(g, refs, info, label):
    """The window's sums against the oracle's per-sample sums added up: N exactly; E and F within quant_bound of the window,
    the rounding of the window's terms to multiples of 2^-k (n terms, each within 2^-(k+1)), and nothing on top of it."""
    N0 = sum(r['N'] for r in refs)
    E0 = sum(r['E'] for r in refs)
    F0 = sum(r['F'] for r in refs)
    assert np.array_equal(g['N'], N0), 'counts differ from the oracle ' + label
    assert g['ungrouped'] == sum(r['ungrouped'] for r in refs)
    dE = np.abs(g['E'] - E0) - quant_bound(N0, info['k_E'])
    dF = np.abs(g['F'] - F0) - quant_bound(N0, info['k_F'])[..., None]
    rel_row(g['E'], E0, tag='field groups E against the oracle')
    rel_row(g['F'], F0, tag='field groups F against the oracle')
    print('%s: largest |E - oracle| less quant_bound %.3e, largest |F - oracle| less quant_bound %.3e (both must be <= 0)'
          % (label, np.max(dE), np.max(dF)))
    assert np.max(dE) <= 0.0 and np.max(dF) <= 0.0


@pytest.mark.parametrize('case', ['ttp', 'ttrrp'])
def test_step_mode_against_oracle(case):
    ct = case_tables(case)
    pop4 = random_population(ct, 20000, seed=5)
    table, G = table_some(ct['M'])
    sim = make_oracle_sim(ct, *pop4, seed=3)
    eng, grid = engine_with_groups(ct, pop4, table, G)
    same_event_rule(eng, sim)
    slots0 = eng.timing()['slots']
    eng.step(30)
    g, f = eng.field_groups(), eng.field()
    refs = []
    for s in range(30):
        sim.run_timestep()
        if (s + 1) % 10 == 0:
            refs.append(oracle_sample(sim, table, G, grid))
    assert g['samples'] == 3 == f['samples']                                # nothing skipped ...
    assert eng.timing()['slots'] == slots0 and eng.timing()['regrows'] == 0   # ... and the store did not grow
    check_window_against_oracle(g, refs, eng.field_groups_info(), case)


# ---------------------------------------------------------------------------------------------- 4. against the band rows
def test_slab_grid_against_band_rows():
    """A slab grid aligned with the slices and the band table as groups: F[slab][g] is k_spectral's F[s][g] of the same step
    (FP64 LDS atomics there, integers here) and N is exact."""
    from nanokappa_amd import spectral as SP
    ct = case_tables('ttp')
    S, a = ct['centers'].shape[0], ct['axis']
    pop4 = random_population(ct, 20000, seed=5)
    band, B, _ = SP.band_map(ct['ph'].omega, 6)
    n = [1, 1, 1]
    n[a] = S
    eng, _ = engine_with_groups(ct, pop4, band, B, n=n)
    eng.set_bands(band, B)
    t = eng.step(10)
    g = eng.field_groups()
    info = eng.field_groups_info()
    assert g['samples'] == 1 and t['band_steps'].tolist() == [9]
    N = np.moveaxis(g['N'], a, 0).reshape(S, B)
    F = np.moveaxis(g['F'], a, 0).reshape(S, B, 3)
    assert np.array_equal(N, t['band_N'][0])
    bound = quant_bound(N, info['k_F'])[..., None] + TOL_ROW_FLUX * np.max(np.abs(t['flux_raw'][9]))
    d = np.abs(F - t['band_F'][0])
    rel_row(F, t['band_F'][0], tag='field groups F against the band rows')
    print('slab grid against the band rows: largest deviation %.3e, bound %.3e' % (d.max(), bound.min()))
    assert np.all(d <= bound)


# ---------------------------------------------------------------------------------------------- 5. paths
def _run_paths(ct, pop4, table, G, flags=0, n=GRID):
    eng, _ = engine_with_groups(ct, pop4, table, G, n=n, flags=flags)
    eng.step(20)
    g = eng.field_groups()
    st = eng.tally_field_groups_state()
    return g, st, eng.field_groups_info()


def test_paths_give_identical_bytes(monkeypatch):
    from nanokappa_amd.engine import FIELD_GLOBAL
    ct = case_tables('ttp')
    pop4 = random_population(ct, 20000, seed=21)
    table, G = table_some(ct['M'])
    r0 = _run_paths(ct, pop4, table, G)
    r1 = _run_paths(ct, pop4, table, G, flags=FIELD_GLOBAL)
    monkeypatch.setenv('NK_FIELD_PATH', 'global')
    r2 = _run_paths(ct, pop4, table, G)
    assert r0[2]['lds_path'] == 1 and r1[2]['lds_path'] == 0 and r2[2]['lds_path'] == 0
    for r in (r1, r2):
        assert r[0]['samples'] == r0[0]['samples'] == 2 and r[0]['ungrouped'] == r0[0]['ungrouped'] > 0
        for k in ('N', 'E', 'F'):
            assert r[0][k].tobytes() == r0[0][k].tobytes(), k
        assert r[1]['raw'].tobytes() == r0[1]['raw'].tobytes()
        assert r[1]['clamped'] == r0[1]['clamped'] and r[1]['ungrouped'] == r0[1]['ungrouped']


def test_large_grid_takes_the_global_path():
    """16 x 16 x 16 cells x 8 groups = 32768 lines (1.2 MB of LDS bins): global integer adds, and the field's integers."""
    ct = case_tables('ttp')
    pop4 = random_population(ct, 20000, seed=23, T0=303.0)
    table, G = table_all(ct['M'], 8)
    eng, _ = engine_with_groups(ct, pop4, table, G, n=(16, 16, 16))
    info = eng.field_groups_info()
    assert info['lds_path'] == 0 and info['lines'] == 16 ** 3 * 8 and info['bytes'] >= info['lines'] * (64 + 40)
    eng.step(10)
    assert_windows_add_up(eng.field(), eng.field_groups())
    assert_groups_add_up_to_field(eng, '(16^3 x 8)')


def test_field_and_groups_choose_their_paths_independently():
    """One engine, one host path for both grids: 16 x 16 x 8 = 2048 cells are 72 KB of LDS bins (above the 64 KB a kernel may
    have without being allowed more, below the 160 KB limit), so the field takes the LDS path; with G = 2 the 4096 lines are
    144 KB -- the LDS path too, with a larger allowance of its own; with G = 8 the 16384 lines do not fit and the groups go
    global while the field stays in LDS.  In either setting the groups' integers add up to the field's, bit for bit."""
    ct = case_tables('ttp')
    pop4 = random_population(ct, 20000, seed=25, T0=303.0)
    table, G = table_all(ct['M'], 2)
    eng, _ = engine_with_groups(ct, pop4, table, G, n=(16, 16, 8))
    for G, paths in ((2, (1, 1)), (8, (1, 0))):
        if G != 2:
            eng.set_field_groups(*table_all(ct['M'], G))
            eng.field(reset=True)                                           # both windows start here
        fi, gi = eng.field_info(), eng.field_groups_info()
        print('G = %d: lds_path field %d, groups %d; %d cells, %d lines' % (G, fi['lds_path'], gi['lds_path'], fi['ncells'], gi['lines']))
        assert fi['ncells'] == 2048 and gi['lines'] == 2048 * G and gi['G'] == G
        assert (fi['lds_path'], gi['lds_path']) == paths
        assert_groups_add_up_to_field(eng, 'G = %d, before stepping' % G)
        eng.step(20)
        f, g = eng.field(), eng.field_groups()
        assert f['samples'] == 2
        assert_windows_add_up(f, g, 'G = %d' % G)
        assert g['N'].sum() == f['N'].sum() > 0 and np.count_nonzero(g['N'].sum(axis=(0, 1, 2))) == G
        assert_groups_add_up_to_field(eng, 'G = %d, after 20 steps' % G)


# ---------------------------------------------------------------------------------------------- 6. a store that regrows
@pytest.mark.parametrize('case', ['ttp', 'ttrrp'])
def test_store_regrows_in_mid_window(case, monkeypatch):
    """Six times the entry rate into a store with hardly any head room: the store grows in mid-window, the table in the
    segments' order is built again, and the window is the oracle's samples added up and the field's window split by group."""
    monkeypatch.setenv('NK_TIGHT_STORE', '1')
    ct = case_tables(case)
    pop4 = random_population(ct, 20000, seed=9)
    table, G = table_all(ct['M'])
    sim = make_oracle_sim(ct, *pop4, seed=3, cap=600000, emit_scale=6.0)
    eng, grid = engine_with_groups(ct, pop4, table, G, emit_scale=6.0)
    same_event_rule(eng, sim)
    slots0, perm0 = eng.timing()['slots'], eng.field_groups_info()['permutes']
    assert perm0 >= 1
    taken = []                              # which of the six field steps became samples (the window is never reset)
    for call in range(6):
        eng.step(10)
        taken.append(eng.field_groups()['samples'])
    taken = np.diff([0] + taken).astype(bool)
    g, f = eng.field_groups(), eng.field()
    assert eng.timing()['slots'] > slots0 and eng.timing()['regrows'] > 0
    assert eng.field_groups_info()['permutes'] > perm0
    assert_windows_add_up(f, g, 'regrown store')                            # the same steps in both windows, whatever was dropped
    assert_groups_add_up_to_field(eng, 'regrown store')
    refs = []
    for s in range(60):
        sim.run_timestep()
        if (s + 1) % 10 == 0:
            refs.append(oracle_sample(sim, table, G, grid))
    # a sample is dropped only where migrants waited in an inbox while the store grew (rough walls); the window is held
    # against the oracle's samples of the steps that were taken, so the comparison is made whatever was dropped
    print('regrown store %s: samples taken at field steps %s' % (case, np.nonzero(taken)[0].tolist()))
    assert g['samples'] == taken.sum() >= 3 and (taken.all() or case == 'ttrrp')
    check_window_against_oracle(g, [r for r, ok in zip(refs, taken) if ok], eng.field_groups_info(), 'regrown store ' + case)


# ---------------------------------------------------------------------------------------------- 7. degenerate shapes
def test_one_group_is_the_field():
    ct = case_tables('ttp')
    pop4 = random_population(ct, 20000, seed=14, T0=303.0)
    eng, _ = engine_with_groups(ct, pop4, np.zeros(ct['M'], dtype=np.int32), 1)
    eng.step(10)
    f, g = eng.field(), eng.field_groups()
    for k in ('N', 'E', 'F'):
        assert g[k][:, :, :, 0].tobytes() == f[k].tobytes(), k
    sf, sg = assert_groups_add_up_to_field(eng, 'G = 1')
    assert np.array_equal(sg['raw'][:, :, :, 0], sf['raw'])


def test_one_cell():
    from nanokappa_amd import field_groups as FG
    ct = case_tables('ttp')
    pop4 = random_population(ct, 20000, seed=15, T0=303.0)
    table, G = table_some(ct['M'])
    eng, (lo, h, n) = engine_with_groups(ct, pop4, table, G, n=(1, 1, 1))
    eng.step(3)
    st = eng.tally_field_groups_state()
    x, e, v = state_on_host(eng, ct)
    grp = table[eng.download()['mode'].astype(int)]
    q = FG.quantised(x, e, v, grp, lo, h, n, G, st['k_E'], st['k_F'])
    assert st['raw'].shape == (1, 1, 1, 3, 8) and np.array_equal(st['raw'], q['raw'])      # (TOL_FIELD_STATE = 0)
    assert st['ungrouped'] == q['ungrouped'] and st['clamped'] == q['clamped']


def test_without_the_partition(monkeypatch):
    """NK_NO_PARTITION=1: the stored index is the mode and the pass reads the caller's table -- no permuted copy is built."""
    monkeypatch.setenv('NK_NO_PARTITION', '1')
    ct = case_tables('ttp')
    pop4 = random_population(ct, 20000, seed=16, T0=303.0)
    table, G = table_all(ct['M'])
    eng, _ = engine_with_groups(ct, pop4, table, G)
    eng.step(10)
    assert eng.field_groups_info()['permutes'] == 0
    assert_windows_add_up(eng.field(), eng.field_groups(), 'no partition')
    sf, sg = assert_groups_add_up_to_field(eng, 'no partition')
    modes = eng.download()['mode'].astype(int)
    assert np.array_equal(sg['raw'][..., 0].sum(axis=(0, 1, 2)), np.bincount(table[modes], minlength=G))


# ---------------------------------------------------------------------------------------------- 8. errors and lifetime
def test_error_paths():
    from nanokappa_amd.engine import NkError, FIELD_TEST_SMALL_BOUND, ERR_ARG
    ct = case_tables('ttp')
    pop4 = random_population(ct, 5000, seed=8, T0=303.0)
    eng = make_engine(ct, *pop4, seed=4)
    table, G = table_some(ct['M'])
    lo, h, n = grid_of(ct)

    def refused(fn, *words):
        with pytest.raises(NkError) as e:
            fn()
        assert 'failed (%d)' % ERR_ARG in str(e.value), str(e.value)
        for w in words:
            assert w in str(e.value), '%r not in %r' % (w, str(e.value))

    refused(lambda: eng.set_field_groups(table, G), 'nk_set_field')                           # groups before a field
    eng.set_field(lo, h, n, 10)
    bad = table.copy()
    bad[7] = G
    refused(lambda: eng.set_field_groups(bad, G), 'group_of_mode[7]', 'outside')
    bad[7] = -2
    refused(lambda: eng.set_field_groups(bad, G), 'group_of_mode[7]', 'outside')
    assert eng.field_groups_info()['on'] == 0 and eng.field_groups_info()['bytes'] == 0
    l2, h2, n2 = grid_of(ct, (64, 64, 64))
    eng.set_field(l2, h2, n2, 10)
    refused(lambda: eng.set_field_groups(np.arange(ct['M'], dtype=np.int32) % 128, 128), 'lines', '2^24')
    # a bound 2^40 times too small: every ordinary term exceeds it -- an error that names the sum, never wrapped integers
    eng.set_field(lo, h, n, 10, flags=FIELD_TEST_SMALL_BOUND)
    eng.set_field_groups(table, G)
    with pytest.raises(NkError, match=r'failed \(-3\).*field groups overflow.*B_E'):          # NK_ERR_CAPACITY
        eng.tally_field_groups_state()
    with pytest.raises(NkError, match='field groups overflow.*B_E'):
        eng.step(10)
    # ... and the engine is usable afterwards
    eng.set_field(lo, h, n, 10)
    eng.set_field_groups(table, G)
    eng.step(10)
    assert eng.field_groups()['samples'] == 1 == eng.field()['samples']


def test_lifetime():
    from nanokappa_amd.engine import NkError, EngineGroup
    ct = case_tables('ttp')
    pop4 = random_population(ct, 5000, seed=8)
    table, G = table_some(ct['M'])
    eng, (lo, h, n) = engine_with_groups(ct, pop4, table, G, seed=4)
    assert eng.field_groups_info()['bytes'] > 0
    eng.set_field_groups(None, 0)                                           # ngroups = 0: everything is freed
    info = eng.field_groups_info()
    assert info['on'] == 0 and info['bytes'] == 0 and info['lines'] == 0
    with pytest.raises(NkError):
        eng.field_groups()
    eng.step(10)
    assert eng.field()['samples'] == 1
    eng.set_field_groups(table, G)
    assert eng.field_groups_info()['on'] == 1
    eng.set_field(lo, h, (0, 0, 0), 10)                                     # the field off: the groups go with it
    assert eng.field_groups_info()['on'] == 0 and eng.field_groups_info()['bytes'] == 0
    with pytest.raises(NkError):
        eng.tally_field_groups_state()
    eng.set_field(lo, h, n, 10)                                             # ... and a new field does not bring them back
    assert eng.field_groups_info()['on'] == 0
    # a replica group refuses a member with groups (through the field's clause)
    other = make_engine(ct, *pop4, seed=5)
    eng2, _ = engine_with_groups(ct, pop4, table, G, seed=6)
    with pytest.raises(NkError) as e:
        EngineGroup([other, eng2])
    assert e.value.code == -2 and 'member 1' in str(e.value) and 'field' in str(e.value)


@pytest.mark.parametrize('case', ['ttp', 'ttrrp'])
def test_groups_leave_everything_else(case):
    """The pass only reads: a run with the groups on gives the history rows and the particles of the same run with the groups
    off -- counts, temperatures, energies and every downloaded particle field bit for bit; the four sums the sweep adds with
    FP64 LDS atomics (E_raw, flux_raw, res_energy, res_flux) are not the same bits in two runs of one engine with the groups
    off either, and are held as such two runs agree (test_gpu_replicas.assert_same_rows, util.RUN_TOL)."""
    from test_gpu_replicas import assert_same_rows
    ct = case_tables(case)
    pop4 = random_population(ct, 20000, seed=8)
    table, G = table_some(ct['M'])
    lo, h, n = grid_of(ct)
    runs = []
    for on in (False, True):
        eng = make_engine(ct, *pop4, seed=4)
        eng.set_field(lo, h, n, 10)
        if on:
            eng.set_field_groups(table, G)
        else:
            assert eng.field_groups_info() == dict(G=0, lines=0, bytes=0, lds_path=0, k_E=0, k_F=0, permutes=0, on=0)
        runs.append((eng.step(25), eng))
    assert sorted(runs[0][0]) == sorted(runs[1][0])
    assert_same_rows(runs[1][0], runs[0][0], 'groups on against off')
    # (rough-wall migrants take their slots in the order the atomics fall: the particles are matched by their ids)
    p, q = runs[1][1].download(), runs[0][1].download()
    i, j = np.argsort(p['pid']), np.argsort(q['pid'])
    for k in ('pid', 'mode', 'facet', 'positions', 'n_timesteps', 'occupation'):
        assert np.array_equal(p[k][i], q[k][j], equal_nan=True), 'downloaded %s differs with the groups on' % k
    assert runs[1][1].field()['N'].tobytes() == runs[0][1].field()['N'].tobytes()


# ---------------------------------------------------------------------------------------------- 9. communicator
def test_through_single_rank_communicator(monkeypatch):
    from nanokappa_amd.engine import comm_unique_id
    ct = case_tables('ttp')
    pop4 = random_population(ct, 20000, seed=9)
    table, G = table_some(ct['M'])
    ref, _ = engine_with_groups(ct, pop4, table, G, seed=1)
    ref.step(20)
    g0, s0 = ref.field_groups(), ref.tally_field_groups_state()
    monkeypatch.setenv('NK_FORCE_COMM', '1')
    pos, mode, occ, counter = pop4
    eng = make_engine(ct, pos, mode, occ, counter, seed=1)
    eng.comm_init(comm_unique_id(), 0, 1)
    lo, h, n = grid_of(ct)
    eng.set_field(lo, h, n, 10)
    eng.set_field_groups(table, G)
    eng.step(20)
    g1, s1 = eng.field_groups(), eng.tally_field_groups_state()
    assert g0['samples'] == g1['samples'] == 2 and g0['ungrouped'] == g1['ungrouped']
    for k in ('N', 'E', 'F'):
        assert g0[k].tobytes() == g1[k].tobytes(), k
    assert s0['raw'].tobytes() == s1['raw'].tobytes() and s0['ungrouped'] == s1['ungrouped']


# ---------------------------------------------------------------------------------------------- 10. Population
def test_population_end_to_end(tmp_path):
    """A parameter-file run with --field_grid 4 2 2 10 --field_groups 4 direction writes field_groups.npz beside field.vtk; the
    file holds what Population.field_groups() returns, and its group heat fluxes add up to the field's."""
    import bench
    from nanokappa_amd import nanokappa, field as FD, field_groups as FG
    argv, species, _ = bench.config_argv('c2', 20000, 200.0)
    argv = argv + ['--seed', '7', '--field_grid', '4', '2', '2', '10', '--field_groups', '4', 'direction', '--iterations', '120',
                   '--results_folder', str(tmp_path / 'run'), '--n_mean', '5']
    pf = tmp_path / 'params.txt'
    pf.write_text(' '.join(argv))
    cwd = os.getcwd()
    os.chdir(str(tmp_path))
    try:
        pop = nanokappa.main(['-ff', str(pf)])
    finally:
        sys.stdout = sys.__stdout__
        os.chdir(cwd)
    path = FG.field_groups_path(pop.results_folder_name)
    assert os.path.exists(path) and os.path.exists(FD.field_path(pop.results_folder_name))
    z, g = FG.read_field_groups(path), pop.field_groups()
    assert z['n'] == (4, 2, 2) == g['n'] and z['kind'] == 'direction' == g['kind'] and z['samples'] == g['samples'] == 5
    assert z['step'] == g['step'] == 100                                    # the latest complete window: steps 51..100
    for k in ('lo', 'h', 'edges', 'N', 'E', 'F', 'heat_flux'):
        assert np.array_equal(z[k], g[k], equal_nan=True), k
    assert z['N'].shape == (4, 2, 2, 4) and z['heat_flux'].shape == (4, 2, 2, 4, 3) and np.all(np.isfinite(z['heat_flux']))
    vtk = FD.read_vtk(FD.field_path(pop.results_folder_name))
    d = np.abs(z['heat_flux'].sum(axis=3) - vtk['heat_flux'])
    assert np.max(d) <= 1e-12 * np.max(np.abs(vtk['heat_flux'])), np.max(d)
    # the map resolves what the field sums: the four direction bins do not carry the same flux
    a = pop.slice_axis
    assert np.ptp(z['heat_flux'][..., a].sum(axis=(0, 1, 2))) > 0
    assert pop.engine.field_groups()['samples'] == pop.engine.field()['samples'] == 2


def test_option_requires_a_field_grid():
    import bench
    from nanokappa_amd import synthetic
    from nanokappa_amd.argument_parser import initialise_parser
    from nanokappa_amd.geometry import Geometry
    from nanokappa_amd.phonon import Phonon
    from nanokappa_amd.population import Population
    argv, species, _ = bench.config_argv('c2', 20000, 200.0)
    args = initialise_parser().parse_args(argv + ['--seed', '3', '--field_groups', '4', 'mfp'])
    args.results_folder = ''
    geo = bench.quiet(Geometry, args)
    ph = Phonon(args, 0, material=synthetic.make_material(31, species, temperatures=np.arange(200.0, 401.0, 10.0)))
    with pytest.raises(ValueError, match='--field_groups requires --field_grid'):
        bench.quiet(Population, args, geo, ph)


def test_window_does_not_depend_on_how_the_run_is_cut():
    """run(70) in one go and in calls of 7 steps: the same windows (30 steps: 3 rows), the same counts per (cell, group); the
    reals as two runs of the engine agree (test_gpu_field.test_window_does_not_depend_on_how_the_run_is_cut)."""
    from test_gpu_field import _field_pop, bench_quiet_run
    out = []
    for pieces in ([70], [7] * 10):
        pop = _field_pop(extra=['--field_groups', '4', 'direction'])
        for k in pieces:
            bench_quiet_run(pop, k)
        out.append((pop.field_groups(), pop.field(), pop.engine.field_groups()))
    (g0, f0, r0), (g1, f1, r1) = out
    assert g0['samples'] == g1['samples'] == 3 == f0['samples'] and r0['samples'] == r1['samples'] == 1
    assert g0['step'] == g1['step'] == 60
    assert np.array_equal(g0['N'], g1['N']) and np.array_equal(r0['N'], r1['N'])
    assert np.max(np.abs(g1['E'] - g0['E'])) <= TOL_RUN_ERAW * np.max(np.abs(g0['E'].sum(axis=3)))
    assert np.max(np.abs(g1['heat_flux'] - g0['heat_flux'])) <= TOL_T * np.max(np.abs(g0['heat_flux']))
