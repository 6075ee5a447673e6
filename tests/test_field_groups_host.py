"""Host side of the grouped field maps (nanokappa_amd/field_groups.py; no GPU): the --field_groups option, the group builders,
the float64 and quantised sums per (cell, group) against field.py's, the normalisation, field_groups.npz, and the C interface's
new symbols."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from util import golden_phonon

from nanokappa_amd import field as FD
from nanokappa_amd import field_groups as FG
from nanokappa_amd import modes as MD
from nanokappa_amd import spectral as SP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'nanokappa_hip.h')
NEW_SYMBOLS = ('nk_set_field_groups', 'nk_get_field_groups', 'nk_tally_field_groups_state', 'nk_field_groups_info')


# ---------------------------------------------------------------------------------------------- 1. the option
def test_option_and_parser():
    from nanokappa_amd.argument_parser import initialise_parser
    assert FG.field_groups_option(None) == (0, None, None) == FG.field_groups_option([]) == FG.field_groups_option(['0'])
    assert FG.field_groups_option(['8', 'frequency']) == (8, 'frequency', None)
    assert FG.field_groups_option(['1', 'branch']) == (1, 'branch', None)
    assert FG.field_groups_option(['12', 'mfp']) == (12, 'mfp', None)
    assert FG.field_groups_option(['4', 'direction']) == (4, 'direction', None)
    assert FG.field_groups_option(['4', 'direction', 'z']) == (4, 'direction', 2)
    assert FG.field_groups_option(['4', 'direction', '1']) == (4, 'direction', 1)
    for bad in (['4'], ['x', 'mfp'], ['-2', 'mfp'], ['4', 'colour'], ['4', 'mfp', 'x'], ['4', 'direction', 'w'],
                ['4', 'direction', 'x', 'y'], ['0', 'mfp']):
        with pytest.raises(ValueError, match='--field_groups: expected G kind'):
            FG.field_groups_option(bad)
    # it lives on the field's grid
    FG.require_field(0, None)
    FG.require_field(4, (8, 4, 4))
    with pytest.raises(ValueError, match='--field_groups requires --field_grid'):
        FG.require_field(4, None)
    p = initialise_parser()
    req = ['--poscar_file', 'POSCAR', '--hdf_file', 'synthetic']
    assert p.parse_args(req).field_groups == [] and FG.field_groups_option(p.parse_args(req).field_groups)[0] == 0
    a = p.parse_args(req + ['--field_grid', '8', '4', '4', '10', '--field_groups', '6', 'direction', 'y'])
    assert FG.field_groups_option(a.field_groups) == (6, 'direction', 1) and FD.field_grid_option(a.field_grid) == ((8, 4, 4), 10)


# ---------------------------------------------------------------------------------------------- 2. the builders
@pytest.mark.parametrize('kind,G', [('frequency', 7), ('branch', 0), ('mfp', 5), ('direction', 6)])
def test_builders_cover_the_active_modes(kind, G):
    ph = golden_phonon()
    inactive = ph.inactive_modes_mask.ravel()
    g, n, edges = FG.build_groups(kind, G, ph, T=300.0, axis=1)
    assert g.dtype == np.int32 and g.shape == (ph.omega.size,) and edges.shape == (n + 1,)
    assert n == (ph.number_of_branches if kind == 'branch' else G)
    assert np.all(g[inactive] == -1) and inactive.any()
    moving = np.linalg.norm(ph.group_vel.reshape(-1, 3), axis=1) > 0
    ok = ~inactive & (moving if kind in ('mfp', 'direction') else True)
    assert np.all((g[ok] >= 0) & (g[ok] < n)) and ok.sum() > n
    assert np.all(g[~ok] == -1)
    assert len(np.unique(g[ok])) > 1 or n == 1


def test_frequency_and_branch_are_the_band_maps():
    ph = golden_phonon()
    act = ~ph.inactive_modes_mask.ravel()
    for kind, G in (('frequency', 9), ('branch', 0)):
        g, n, edges = FG.build_groups(kind, G, ph)
        b, nb, eb = SP.band_map(ph.omega, G, kind)
        assert n == nb and np.array_equal(edges, eb) and np.array_equal(g[act], b[act])
    # ... and without a mask, on every mode
    g, n, edges = FG.frequency_groups(ph.omega, 9)
    assert np.array_equal(g, SP.band_map(ph.omega, 9)[0])


def test_direction_groups():
    ph = golden_phonon()
    v = ph.group_vel.reshape(-1, 3)
    for axis in (0, 1, 2):
        g, n, edges = FG.direction_groups(v, 2, axis)
        assert n == 2 and np.array_equal(edges, [-1.0, 0.0, 1.0])
        assert np.all(g[v[:, axis] < 0] == 0) and np.all(g[v[:, axis] > 0] == 1)         # the sign of v . axis
        still = np.linalg.norm(v, axis=1) == 0
        assert np.all(g[still] == -1) and np.all(g[~still] >= 0)
    # a vector as axis; uniform bins of the cosine, the last one closed
    vv = np.array([[1.0, 0, 0], [-1.0, 0, 0], [0, 1.0, 0], [1.0, 1.0, 0], [0, 0, 0], [-1.0, 1e-9, 0]])
    g, _, _ = FG.direction_groups(vv, 4, (2.0, 0.0, 0.0))
    assert g.tolist() == [3, 0, 2, 3, -1, 0]
    g, _, _ = FG.direction_groups(vv, 4, 0, inactive=np.array([1, 0, 0, 0, 0, 0], dtype=bool))
    assert g.tolist() == [-1, 0, 2, 3, -1, 0]


def test_mfp_groups():
    ph = golden_phonon()
    T = 300.0
    mfp = MD.mean_free_path(ph, T)
    g, n, edges = FG.build_groups('mfp', 8, ph, T=T)
    inactive = ph.inactive_modes_mask.ravel()
    x = mfp.ravel()
    ok = ~inactive & (x > 0) & np.isfinite(x)
    assert np.all(np.diff(np.log(edges)) > 0) and np.allclose(np.diff(np.log(edges)), np.diff(np.log(edges))[0], rtol=1e-12)
    assert edges[0] == x[ok].min() and edges[-1] == x[ok].max()
    assert np.all((x[ok] >= edges[g[ok]]) & (x[ok] <= edges[g[ok] + 1]))
    assert g[ok][np.argmax(x[ok])] == 7 and g[ok][np.argmin(x[ok])] == 0
    # the temperature is clipped into the material's range; 'mfp' needs one
    lo = float(ph.temperature_array[0])
    assert np.array_equal(FG.build_groups('mfp', 8, ph, T=lo - 50.0)[0], FG.build_groups('mfp', 8, ph, T=lo)[0])
    with pytest.raises(ValueError, match='temperature'):
        FG.build_groups('mfp', 8, ph)
    with pytest.raises(ValueError, match='unknown group kind'):
        FG.build_groups('colour', 8, ph)
    # nothing moves: every mode is ungrouped
    g0, _, e0 = FG.mfp_groups(np.zeros(10), 4)
    assert np.all(g0 == -1) and np.all(np.isnan(e0))


# ---------------------------------------------------------------------------------------------- 3. the sums
def _particles(P=20000, seed=3, G=5, ungrouped=False):
    rng = np.random.default_rng(seed)
    lo, h, n = np.array([-1.0, 0.0, 2.0]), np.array([0.4, 1.0, 0.7]), (5, 3, 2)
    pos = lo + rng.random((P, 3)) * h * np.array(n) * 1.02 - 0.01 * h * np.array(n)      # a few outside: clamped
    e = rng.standard_normal(P) * 1e-3
    v = rng.standard_normal((P, 3)) * 50.0
    grp = rng.integers(-1 if ungrouped else 0, G, P)
    return pos, e, v, grp, lo, h, n, G


def test_quantised_sums_over_the_groups_equal_the_field():
    pos, e, v, grp, lo, h, n, G = _particles()
    for kE, kF in ((60, 50), (30, 20), (12, 3)):
        q = FG.quantised(pos, e, v, grp, lo, h, n, G, kE, kF)
        f = FD.quantised(pos, e, v, lo, h, n, kE, kF)
        assert q['raw'].dtype == np.int64 and q['raw'].shape == n + (G, 8)
        assert np.array_equal(q['raw'].sum(axis=3), f['raw'])                            # bit for bit
        assert q['clamped'] == f['clamped'] > 0 and q['ungrouped'] == 0
    # one group IS the field; a single particle lands in one line
    q1 = FG.quantised(pos, e, v, np.zeros_like(grp), lo, h, n, 1, 40, 30)
    assert np.array_equal(q1['raw'][:, :, :, 0], FD.quantised(pos, e, v, lo, h, n, 40, 30)['raw'])
    one = FG.quantised(pos[:1], e[:1], v[:1], grp[:1], lo, h, n, G, 40, 30)
    c = FD.cell_index(pos[:1], lo, h, n)[0][0]
    assert one['raw'][..., 0].sum() == 1 and one['raw'][c[0], c[1], c[2], grp[0], 0] == 1


def test_float_sums_and_ungrouped_particles():
    pos, e, v, grp, lo, h, n, G = _particles(ungrouped=True)
    r = FG.groups_from_particles(pos, e, v, grp, lo, h, n, G)
    ok = grp >= 0
    f = FD.field_from_particles(pos[ok], e[ok], v[ok], lo, h, n)
    assert r['ungrouped'] == int((~ok).sum()) > 0 and r['clamped'] == f['clamped']
    assert np.array_equal(r['N'].sum(axis=3), f['N']) and r['N'].sum() == ok.sum()
    assert np.allclose(r['E'].sum(axis=3), f['E'], rtol=0, atol=1e-15) and np.allclose(r['F'].sum(axis=3), f['F'], rtol=0, atol=1e-11)
    for g in range(G):
        m = grp == g
        fg = FD.field_from_particles(pos[m], e[m], v[m], lo, h, n)
        assert np.array_equal(r['N'][..., g], fg['N']) and np.array_equal(r['E'][..., g], fg['E']) and np.array_equal(r['F'][..., g, :], fg['F'])
    # the quantised sums stay within the rounding of the terms
    q = FG.quantised(pos, e, v, grp, lo, h, n, G, 40, 25)
    assert np.array_equal(q['N'], r['N']) and q['ungrouped'] == r['ungrouped']
    assert np.all(np.abs(q['E'] - r['E']) <= r['N'] * np.ldexp(1.0, -41) + 1e-17)
    assert np.all(np.abs(q['F'] - r['F']) <= r['N'][..., None] * np.ldexp(1.0, -26) + 1e-13)
    for bad in (np.full_like(grp, G), np.full_like(grp, -2), grp[:-1]):
        with pytest.raises(ValueError, match='one group'):
            FG.groups_from_particles(pos, e, v, bad, lo, h, n, G)


def test_normalised_groups_add_up_to_the_field():
    pos, e, v, grp, lo, h, n, G = _particles(P=5000)
    r = FG.groups_from_particles(pos, e, v, grp, lo, h, n, G)
    f = FD.field_from_particles(pos, e, v, lo, h, n)
    kw = dict(particle_density=0.01, cell_volume=float(np.prod(h)))
    for norm in ('mean', 'fixed'):
        a = FG.normalise(r['N'], r['E'], r['F'], f['N'], 4, 1000, 7.5, 1.6e13, norm=norm, **kw)
        b = FD.normalise(f['N'], f['E'], f['F'], 4, 1000, 7.5, 1.6e13, norm=norm, **kw)
        assert a['heat_flux'].shape == n + (G, 3) and a['energy'].shape == n + (G,)
        assert np.max(np.abs(a['heat_flux'].sum(axis=3) - b['heat_flux'])) <= 1e-12 * np.max(np.abs(b['heat_flux']))
        assert np.max(np.abs(a['energy'].sum(axis=3) - b['energy'])) <= 1e-12 * np.max(np.abs(b['energy']))
        assert np.array_equal(a['N'].sum(axis=3), b['N'])
    # an empty cell is NaN in every group
    N0 = f['N'].copy()
    N0[0, 0, 0] = 0
    assert np.all(np.isnan(FG.normalise(r['N'], r['E'], r['F'], N0, 4, 1000, 7.5, 1.0)['heat_flux'][0, 0, 0]))
    with pytest.raises(ValueError):
        FG.normalise(r['N'], r['E'], r['F'], f['N'], 4, 1000, 7.5, 1.0, norm='fixed')


# ---------------------------------------------------------------------------------------------- 4. the file
def test_npz_round_trip(tmp_path):
    rng = np.random.default_rng(5)
    n, G = (4, 3, 2), 6
    lo, h = np.array([0.0, -1.0, 2.0]), np.array([1.0, 0.5, 0.25])
    N, E = rng.integers(0, 9, n + (G,)).astype(float), rng.standard_normal(n + (G,))
    F, hf = rng.standard_normal(n + (G, 3)), rng.standard_normal(n + (G, 3))
    hf[0, 0, 0] = np.nan
    edges = np.linspace(-1, 1, G + 1)
    path = FG.write_field_groups(FG.field_groups_path(str(tmp_path)), lo, h, n, 'direction', edges, N, E, F, hf, 5, 250)
    assert os.path.basename(path) == 'field_groups.npz'
    z = FG.read_field_groups(path)
    assert sorted(z) == sorted(('lo', 'h', 'n', 'kind', 'edges', 'N', 'E', 'F', 'heat_flux', 'samples', 'step'))
    assert z['n'] == n and z['kind'] == 'direction' and z['samples'] == 5 and z['step'] == 250
    for k, a in (('lo', lo), ('h', h), ('edges', edges), ('N', N), ('E', E), ('F', F), ('heat_flux', hf)):
        assert np.array_equal(z[k], a, equal_nan=True), k


# ---------------------------------------------------------------------------------------------- 5. the C interface
def test_header_stays_plain_c():
    subprocess.check_call(['gcc', '-std=c99', '-fsyntax-only', '-x', 'c', HEADER])
    hdr = open(HEADER).read()
    assert 'int nk_set_field_groups(nk_ctx *ctx, int32_t ngroups, const int32_t *group_of_mode);' in hdr
    assert 'int nk_tally_field_groups_state(nk_ctx *ctx, int64_t *raw, int64_t *clamped, int64_t *ungrouped);' in hdr
    assert '} nk_field_groups_report;' in hdr


def test_new_symbols_are_exported():
    from nanokappa_amd import engine
    if not os.path.exists(engine.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    L = engine.load_library()
    hdr = open(HEADER).read()
    for name in NEW_SYMBOLS:
        assert name in engine.EXPORTS and hasattr(L, name), 'library does not export %s' % name
        assert 'int %s(nk_ctx *' % name in hdr
    assert C.sizeof(engine.nk_field_groups_report) == 48
    for m in ('set_field_groups', 'field_groups', 'tally_field_groups_state', 'field_groups_info'):
        assert callable(getattr(engine.Engine, m))
