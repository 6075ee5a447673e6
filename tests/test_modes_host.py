"""Host side of the mode-resolved tally (nanokappa_amd/modes.py; no GPU): the float64 table against the reference's own frozen
step, the quantised sums, mode_k against spectral.connection_k for any band table, the accumulation, the mean free path, the
text output, the --mode_tally option, the C interface's new symbols, and the shape of the compiled kernels (gfx950 assembly)."""
import os
import re
import shutil
import subprocess
import sys
import tempfile

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from util import golden, sub, golden_phonon, TOL_E

from nanokappa_amd import modes as MD
from nanokappa_amd import spectral as SP
from nanokappa_amd.constants import Constants

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = '/opt/rocm/bin/hipcc'
K = Constants()


def frozen(variant='lin'):
    """Particles of the frozen step (tests/golden/step.npz) where calculate_energy saw them: subvolume, global mode, e_i."""
    gs = sub(golden('step'), variant)
    gm = sub(golden('mesh'), 'box200ttp')
    ph = golden_phonon()
    m = gs['mid_modes']
    mode = m[:, 0] * ph.number_of_branches + m[:, 1]
    return gs, gm, ph, gs['post_subvol_id'].astype(int), mode.astype(int), gs['energies']


# ---------------------------------------------------------------------------------------------- 1. the reference's frozen step
@pytest.mark.parametrize('variant', ['lin', 'near', 'fixed', 'tref'])
def test_table_against_the_frozen_step(variant):
    from nanokappa_amd import field as FD
    gs, gm, ph, sv, mode, e = frozen(variant)
    S, M = int(gm['n_of_subvols']), ph.number_of_qpoints * ph.number_of_branches
    t = MD.table_from_particles(sv, mode, e, S, M)
    assert t['N'].shape == t['E'].shape == (S, M)
    # every particle lands in exactly one bin
    assert t['N'].sum() == sv.shape[0] and np.array_equal(t['N'][sv, mode] >= 1, np.ones(sv.shape[0], dtype=bool))
    one = MD.table_from_particles(sv[:1], mode[:1], e[:1], S, M)
    assert one['N'].sum() == 1 and one['N'][sv[0], mode[0]] == 1 and one['E'][sv[0], mode[0]] == e[0]
    assert np.array_equal(t['N'].sum(axis=1), gs['post_subvol_N_p'])
    # the reference's normalisation of the subvolume sums (calculate_energy, calculate_heat_flux), as test_field_host.py
    if variant == 'tref':
        ref = np.full(S, float(ph.crystal_energy_function(300.0)))
    else:
        ref = np.asarray(ph.crystal_energy_function(gs['mid_subvol_temperature']))
    F = MD.mode_flux(t['E'], ph.group_vel).sum(axis=1)
    vol = float(np.prod((gm['bounds'][1] - gm['bounds'][0]))) / S
    out = FD.normalise(t['N'].sum(axis=1), t['E'].sum(axis=1), F, 1, ph.number_of_active_modes, ph.number_of_qpoints * ph.volume_unitcell,
                       K.eVpsa2_in_Wm2, norm=('fixed' if variant == 'fixed' else 'mean'), particle_density=float(gs['particle_density']),
                       cell_volume=vol, ref_energy=ref)
    assert np.max(np.abs(out['energy'] - gs['post_subvol_energy']) / np.abs(gs['post_subvol_energy'])) <= TOL_E
    assert np.max(np.abs(out['heat_flux'] - gs['heat_flux'])) <= 1e-12 * np.max(np.abs(gs['heat_flux']))
    with pytest.raises(ValueError):
        MD.table_from_particles(sv, mode, e, S, int(mode.max()))                                # a mode outside the table


# ---------------------------------------------------------------------------------------------- 2. the quantised sums
def test_quantised_against_the_float_sums_and_splits():
    gs, gm, ph, sv, mode, e = frozen('lin')
    S, M = int(gm['n_of_subvols']), ph.number_of_qpoints * ph.number_of_branches
    t = MD.table_from_particles(sv, mode, e, S, M)
    for k in (50, 30, 12):
        q = MD.quantised(sv, mode, e, S, M, k)
        assert q['N_raw'].dtype == q['E_raw'].dtype == np.int64 and np.array_equal(q['N'], t['N'])
        slack = 1e-15 * np.max(np.abs(t['E']))                                       # (the float sums' own rounding)
        assert np.all(np.abs(q['E'] - t['E']) <= t['N'] * np.ldexp(1.0, -(k + 1)) + slack)
    # two disjoint halves add up to the whole, bit for bit; the order of the particles does not matter
    p = np.random.default_rng(1).permutation(sv.shape[0])
    h = sv.shape[0] // 3
    a, b = p[:h], p[h:]
    qa, qb, qw = MD.quantised(sv[a], mode[a], e[a], S, M, 50), MD.quantised(sv[b], mode[b], e[b], S, M, 50), MD.quantised(sv, mode, e, S, M, 50)
    assert np.array_equal(qa['E_raw'] + qb['E_raw'], qw['E_raw']) and np.array_equal(qa['N_raw'] + qb['N_raw'], qw['N_raw'])
    assert np.array_equal(MD.quantised(sv[p], mode[p], e[p], S, M, 50)['E_raw'], qw['E_raw'])
    assert np.abs(qw['E_raw']).max() > 0


# ---------------------------------------------------------------------------------------------- 3. mode_k and bands
def test_mode_k_summed_by_band_is_connection_k_of_the_band_sums():
    gs, gm, ph, sv, mode, e = frozen('lin')
    kc = golden('k_contribution')
    S, M = int(gm['n_of_subvols']), ph.number_of_qpoints * ph.number_of_branches
    t = MD.table_from_particles(sv, mode, e, S, M)
    con, cv, T = kc['subvol_connections'], kc['subvol_con_vectors'], kc['mean_T']
    am, qv = int(kc['number_of_active_modes']), ph.number_of_qpoints * ph.volume_unitcell
    km = MD.mode_k(t['E'], t['N'], ph.group_vel, con, cv, T, am, qv, K.eVpsa2_in_Wm2, K.a_in_m)
    assert km.shape == (con.shape[0], M)
    n_sv = t['N'].sum(axis=1)
    rng = np.random.default_rng(5)
    holes = (rng.permutation(M) % 37).astype(np.int32)
    holes[rng.random(M) < 0.25] = -1
    for band, B in ((SP.frequency_bands(ph.omega, 100)[0], 100), (holes, 37)):
        F = np.moveaxis(MD.band_sums(np.moveaxis(MD.mode_flux(t['E'], ph.group_vel), 2, 1), band, B), 1, 2)     # [S, B, 3]
        N = MD.band_sums(t['N'], band, B)
        kb = SP.connection_k(F, N, con, cv, T, am, qv, K.eVpsa2_in_Wm2, K.a_in_m, n_sv=n_sv)
        ks = MD.band_sums(km, band, B)
        # k is linear in F: the two are sums of the same products in two orders -- within n_band 2^-52 sum |k_m| per band
        # (each product k_m carries a few roundings of its own: three products and two sums per mode, counted into the n)
        nb = np.bincount(band[band >= 0], minlength=B)
        bound = (nb + 8) * np.ldexp(1.0, -52) * MD.band_sums(np.abs(km), band, B)
        assert np.all(np.abs(ks - kb) <= bound), float(np.max(np.abs(ks - kb) / np.maximum(bound, 1e-300)))
    # frequency bands hold every mode: the golden k(omega) of the reference itself
    ks = MD.band_sums(km, SP.frequency_bands(ph.omega, 100)[0], 100)
    e_post = ph.hbar * ph.omega.ravel()[mode] * (gs['post_occupation'] - ph.calculate_occupation(gs['post_temperatures'], ph.omega.ravel()[mode]))
    tp = MD.table_from_particles(sv, mode, e_post, S, M)
    kp = MD.band_sums(MD.mode_k(tp['E'], tp['N'], ph.group_vel, con, cv, T, am, qv, K.eVpsa2_in_Wm2, K.a_in_m),
                      SP.frequency_bands(ph.omega, 100)[0], 100)
    assert np.max(np.abs(kp - kc['y'])) <= 1e-12 * np.max(np.abs(kc['y']))
    # occupation deviation: E / (hbar omega N), NaN in empty bins
    dn = MD.occupation_deviation(tp['E'], tp['N'], ph.omega, ph.hbar)
    i = 7
    assert dn[sv[i], mode[i]] == pytest.approx(tp['E'][sv[i], mode[i]] / (ph.hbar * ph.omega.ravel()[mode[i]] * tp['N'][sv[i], mode[i]]), rel=1e-15)
    assert np.isnan(dn[tp['N'] == 0]).all() and np.isfinite(dn[tp['N'] > 0]).all()


# ---------------------------------------------------------------------------------------------- 4. accumulation, mfp, files, option
def test_accumulation_against_brute_force():
    rng = np.random.default_rng(2)
    C, M = 3, 200
    k = rng.standard_normal((C, M))
    x = rng.integers(0, 40, M).astype(float)              # many ties
    grid = np.array([-1.0, 0.0, 0.0, 3.5, 7.0, 7.0, 39.0, 100.0])
    acc = MD.accumulation(k, x, grid)
    assert acc.shape == (C, grid.shape[0])
    order = np.argsort(x, kind='stable')
    cs = np.cumsum(k[:, order], axis=1)
    for i, g in enumerate(grid):
        n = int(np.sum(x <= g))                            # ties in x counted once, all of them
        want = cs[:, n - 1] if n else np.zeros(C)
        assert np.allclose(acc[:, i], want, rtol=0, atol=1e-13)
    assert np.all(acc[:, 0] == 0.0) and np.array_equal(acc[:, 1], acc[:, 2])
    assert np.allclose(acc[:, -1], k.sum(axis=1), rtol=0, atol=1e-13) and np.array_equal(acc[:, -1], acc[:, -2])
    assert MD.accumulation(k[0], x, grid).shape == grid.shape
    with pytest.raises(ValueError, match='decrease'):
        MD.accumulation(k, x, [0.0, 2.0, 1.0])
    with pytest.raises(ValueError):
        MD.accumulation(k, x[:-1], grid)
    g = MD.accumulation_grid(x, 50)
    assert np.all(np.diff(g) > 0) and g[-1] == x.max() and g[0] == x[x > 0].min()
    assert np.allclose(MD.accumulation(k, x, g)[:, -1], k.sum(axis=1), rtol=0, atol=1e-13)
    # a NaN x (a mode without a lifetime) is in no point
    x2 = x.copy()
    x2[5] = np.nan
    assert np.allclose(MD.accumulation(k, x2, [100.0])[:, 0], k.sum(axis=1) - k[:, 5], rtol=0, atol=1e-13)


def test_mean_free_path_against_the_lifetime_function():
    ph = golden_phonon()
    Q, J = ph.omega.shape
    for T in (300.0, float(ph.temperature_array[0]), 0.5 * float(ph.temperature_array[3] + ph.temperature_array[4])):
        mfp = MD.mean_free_path(ph, T)
        assert mfp.shape == (Q, J)
        rng = np.random.default_rng(3)
        for q, j in zip(rng.integers(0, Q, 50), rng.integers(0, J, 50)):
            tau = ph.lifetime_function(np.array([[T, q, j]]))[0]
            # (the norm of one vector and of a whole array add the three squares in different orders: a few units in the last place)
            assert mfp[q, j] == pytest.approx(np.linalg.norm(ph.group_vel[q, j]) * tau, rel=4 * 2.0 ** -52, abs=0)
    assert np.all(mfp >= 0) and mfp.max() > 0


def test_files_round_trip(tmp_path):
    rng = np.random.default_rng(4)
    con = np.array([[0, 1], [1, 2], [2, 3]])
    grid = np.geomspace(1.0, 1e5, 17)
    cum = np.cumsum(rng.standard_normal((3, 17)), axis=1)
    for by in ('mfp', 'frequency'):
        path = MD.write_k_accumulation(MD.k_accumulation_path(str(tmp_path), by), grid, cum, con, by=by, steps=300)
        lines = open(path).read().splitlines()
        assert lines[0].startswith('# conductivity accumulated over the ' + ('mean free path' if by == 'mfp' else 'frequency'))
        assert lines[1].split()[1:] == ['mean_free_path' if by == 'mfp' else 'omega', 'cum_k_0-1', 'cum_k_1-2', 'cum_k_2-3']
        g, c = MD.read_k_accumulation(path)
        assert np.array_equal(g, grid) and np.array_equal(c, cum)           # (%.17e: exact)
    assert os.path.basename(MD.k_accumulation_path('x')) == 'k_accumulation.txt'
    ph = golden_phonon()
    Q, J = ph.omega.shape
    N, E = rng.integers(0, 5, (4, Q, J)).astype(float), rng.standard_normal((4, Q * J))
    path = MD.write_mode_tally(MD.mode_tally_path(str(tmp_path)), N, E, 5, 250, ph.omega, ph.group_vel)
    z = MD.read_mode_tally(path)
    assert os.path.basename(path) == 'mode_tally.npz' and z['N'].shape == z['E'].shape == (4, Q, J)
    assert np.array_equal(z['N'], N) and np.array_equal(z['E'].reshape(4, -1), E) and int(z['samples']) == 5 and int(z['step']) == 250
    assert np.array_equal(z['omega'], ph.omega) and np.array_equal(z['group_vel'], ph.group_vel)


def test_mode_tally_option_and_parser():
    from nanokappa_amd.argument_parser import initialise_parser
    assert MD.mode_tally_option(None) == 0 and MD.mode_tally_option([]) == 100 and MD.mode_tally_option(['10']) == 10
    assert MD.mode_tally_option(['200'], 10) == 200 and MD.mode_tally_option('50') == 50
    assert MD.mode_tally_option(['0']) == 0
    for bad in (['15'], ['-10'], ['x'], ['10', '20'], ['5']):
        with pytest.raises(ValueError, match='--mode_tally'):
            MD.mode_tally_option(bad)
    p = initialise_parser()
    req = ['--poscar_file', 'POSCAR', '--hdf_file', 'synthetic']
    assert p.parse_args(req).mode_tally == ['0'] and MD.mode_tally_option(p.parse_args(req).mode_tally) == 0
    assert MD.mode_tally_option(p.parse_args(req + ['--mode_tally']).mode_tally) == 100
    assert MD.mode_tally_option(p.parse_args(req + ['--mode_tally', '10', '--n_mean', '5']).mode_tally) == 10
    with pytest.raises(ValueError, match='--mode_tally'):
        MD.mode_tally_option(p.parse_args(req + ['--mode_tally', '25']).mode_tally)


# ---------------------------------------------------------------------------------------------- 5. the C interface
def test_new_symbols_are_declared_and_exported():
    from nanokappa_amd import engine
    hdr = open(os.path.join(ROOT, 'include', 'nanokappa_hip.h')).read()
    src = open(os.path.join(ROOT, 'nanokappa_amd', 'csrc', 'nk_engine.hip')).read()
    for n in ('nk_set_modes', 'nk_get_modes', 'nk_tally_modes_state', 'nk_modes_info'):
        assert n in engine.EXPORTS
        assert 'int %s(nk_ctx *' % n in hdr and 'int %s(nk_ctx *' % n in src
    assert engine.MODES_GLOBAL == 1 and engine.MODES_TEST_SMALL_BOUND == 2
    assert '#define NK_MODES_GLOBAL 1' in hdr and '#define NK_MODES_TEST_SMALL_BOUND 2' in hdr
    import ctypes as C
    assert C.sizeof(engine.nk_modes) == 16 and C.sizeof(engine.nk_modes_report) == 40


# ---------------------------------------------------------------------------------------------- 6. the shape of the kernels
_ASM = {}


def _assembly():
    """nk_modes.hip compiled to gfx950 assembly with the flags of nanokappa_amd/csrc/Makefile (CXXFLAGS); no GPU needed."""
    if 'text' not in _ASM:
        assert os.path.exists(HIPCC), 'hipcc is required here: the check is part of the build'
        tmp = tempfile.mkdtemp()
        try:
            out = os.path.join(tmp, 'nk_modes.s')
            subprocess.check_call([HIPCC, '--offload-arch=gfx950', '-O3', '-std=c++17', '-munsafe-fp-atomics', '-mllvm', '-disable-machine-licm',
                                   '--cuda-device-only', '-S', '-o', out, os.path.join(ROOT, 'nanokappa_amd', 'csrc', 'nk_modes.hip')],
                                  stderr=subprocess.DEVNULL)
            _ASM['text'] = open(out).read()
        finally:
            shutil.rmtree(tmp, ignore_errors=True)
    return _ASM['text']


def _kernel(text, name):
    lines = text.split('\n')
    a = next((i for i, l in enumerate(lines) if l.startswith(name + ':')), None)
    assert a is not None, 'kernel %s not found in the assembly' % name
    b = next(i for i in range(a, len(lines)) if '.end_amdhsa_kernel' in lines[i])
    return [l.split(';')[0].strip() for l in lines[a:b]], '\n'.join(lines[a:b])


@pytest.mark.parametrize('state', [False, True])
def test_kernel_shape(state):
    text = _assembly()
    name = '_Z7k_modesILb%dEEv5NkDev10NkModesDev' % (1 if state else 0)
    code, raw = _kernel(text, name)
    ops = [c.split()[0] for c in code if c and not c.startswith('.') and not c.endswith(':')]
    assert 'ds_add_u64' in ops and 'ds_add_u32' in ops                      # the owner path's bins: integer LDS adds
    assert 'global_atomic_add_x2' in ops and 'global_atomic_add' in ops     # the global path and the header: integer adds
    assert not [o for o in ops if 'cmpswap' in o], 'a compare-and-swap loop'
    fp_atomic = re.compile(r'atomic_(add|pk_add|min|max|fmin|fmax)_(f16|f32|f64|bf16)|ds_(add|min|max|pk_add)_(rtn_)?(f16|f32|f64|bf16)')
    assert not [o for o in ops if fp_atomic.search(o)], 'a floating-point atomic'
    # no scratch: a spilled register in a streaming loop is reloaded through the same in-order queue as the next loads
    assert not [o for o in ops if o.startswith('scratch_') or o.startswith('buffer_') and 'offen' in o]
    assert re.search(r'\.amdhsa_private_segment_fixed_size 0\b', raw), 'the kernel uses scratch memory'
    meta = re.search(r'\.name:\s+%s\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)' % re.escape(name), text)
    assert meta is None or int(meta.group(1)) == 0


def test_only_the_modes_kernels_are_in_the_translation_unit():
    text = _assembly()
    names = set(re.findall(r'^\s*\.amdhsa_kernel\s+(\S+)', text, flags=re.M))
    assert len(names) == 4 and all('k_modes' in n for n in names), names
