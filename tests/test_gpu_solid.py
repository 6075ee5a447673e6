"""Solid fraction of the field's cells on the GPU (nk_cell_solid_volume: k_solid_clip, k_solid_finish) against the host
restatement field.solid_volume: the shapes of test_solid_host.py, the 5000-face STL wire, the error paths, and the
Population outputs with and without --field_solid."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from util import allclose, rel_err
from solid_cases import case

pytestmark = pytest.mark.gpu

# Device against host, in units of the cell volume.  Both sides form the same terms a and p with the same operations (the
# kernels are compiled without multiply-add contraction); the device then rounds each term to a multiple of 2^-k (k = 62 -
# ceil(log2 n_faces): 2^-57 for 28 faces, 2^-49 for 5000) and adds integers, the host adds doubles in another order.
# Measured on an MI355X (`solid ... device against host (cells)` in the parity margins): 0 (box) .. 3.33e-16 cells on the
# primitives, 2.67e-14 (16 x 16 x 32) and 3.86e-14 (one cell) on the 5000-face wire -- the integers' rounding, 2^-50 per term,
# over the terms of a cell.  bound = 10 x measured, and never above 1e-9 cells.
TOL_SOLID = 3.3e-15         # the primitives, 12 .. 216 faces       (measured <= 3.33e-16)
TOL_SOLID_WIRE = 3.8e-13    # the STL wire, 5000 faces               (measured 2.67e-14, 3.86e-14)
assert TOL_SOLID <= 1e-9 and TOL_SOLID_WIRE <= 1e-9

# (shape, cells, cells added on every side): box, 7-sided cylinder, the concave star (several crossings per ray, empty cells),
# corrugated, the turned castle with and without grid planes on its lids, the enlarged grid, and one cell for the whole mesh
DEVICE_CASES = [('box', (3, 2, 2), 0), ('cyl7', (5, 3, 2), 0), ('star', (5, 5, 2), 0), ('corrugated', (3, 4, 5), 0),
                ('turned_castle', (5, 3, 3), 0), ('turned_castle', (4, 3, 3), 0), ('cyl7', (5, 3, 2), 1), ('star', (5, 5, 2), 1),
                ('cyl7', (1, 1, 1), 0)]


@pytest.mark.parametrize('name,n,pad', DEVICE_CASES)
def test_device_against_host(name, n, pad):
    from nanokappa_amd import engine, field as FD
    m, lo, h, n = case(name, n, pad)
    V, rep = engine.cell_solid_volume(m.vertices, m.faces, lo, h, n, report=True)
    H = FD.solid_volume(m.vertices, m.faces, lo, h, n)
    cv = float(np.prod(h))
    assert V.shape == H.shape == n and rep['ncells'] == n[0] * n[1] * n[2] and rep['pairs'] >= m.faces.shape[0]
    print('%s %s pad %d: largest |device - host| = %.3e cells, k_A %d' % (name, n, pad, np.abs(V - H).max() / cv, rep['k_A']))
    assert allclose(V / cv, H / cv, rtol=0.0, atol=TOL_SOLID, tag='solid %s device against host (cells)' % name)
    assert rel_err(V.sum(), m.volume, tag='solid %s closure' % name) <= 1e-12
    fr = V / cv
    assert fr.min() >= -1e-12 and fr.max() <= 1.0 + 1e-12
    if name == 'box':
        assert np.all(np.abs(fr - 1.0) <= 1e-12)
    if name == 'star':
        assert (fr <= 1e-12).sum() >= 1
    if pad:
        outer = V.copy()
        outer[pad:-pad, pad:-pad, pad:-pad] = 0.0
        assert np.all(np.abs(outer) <= 1e-12 * cv)          # (a vertex a rounding below the first inner plane leaves ~1e-15)
    if n == (1, 1, 1):
        assert abs(V[0, 0, 0] - m.volume) <= 1e-12 * m.volume


_WIRE = {}


def wire_mesh():
    """The 5000-face STL wire of the benchmark's config 4 (built once)."""
    if not _WIRE:
        import bench
        args, geo = bench.wire_geometry(200000)
        _WIRE.update(v=np.array(geo.mesh.vertices), f=np.array(geo.mesh.faces), bounds=np.array(geo.bounds), volume=float(geo.mesh.volume))
    return _WIRE


def test_wire():
    """16 x 16 x 32 cells over the wire: closure, range, two calls the same bytes, every cell against the host."""
    from nanokappa_amd import engine, field as FD
    w = wire_mesh()
    assert w['f'].shape[0] == 5000
    lo, h, n = FD.grid_from_bounds(w['bounds'], (16, 16, 32))
    V, rep = engine.cell_solid_volume(w['v'], w['f'], lo, h, n, report=True)
    V2 = engine.cell_solid_volume(w['v'], w['f'], lo, h, n)
    assert V.tobytes() == V2.tobytes()
    cv = float(np.prod(h))
    fr = V / cv
    assert rel_err(V.sum(), w['volume'], tag='solid wire closure') <= 1e-12
    assert fr.min() >= -1e-12 and fr.max() <= 1.0 + 1e-12
    assert (fr <= 1e-12).sum() >= 1 and (np.abs(fr - 1.0) <= 1e-12).sum() >= 1          # corner cells outside, core cells full
    H = FD.solid_volume(w['v'], w['f'], lo, h, n)
    print('wire %s: largest |device - host| = %.3e cells, pairs %d, k_A %d, %.3g s on the device'
          % (n, np.abs(V - H).max() / cv, rep['pairs'], rep['k_A'], rep['seconds']))
    assert allclose(fr, H / cv, rtol=0.0, atol=TOL_SOLID_WIRE, tag='solid wire device against host (cells)')


def test_wire_in_one_cell():
    """The same mesh on a 1 x 1 x 1 grid: all 5000 faces add into one line (contention, and the scale's bound: 5000 terms)."""
    from nanokappa_amd import engine, field as FD
    w = wire_mesh()
    lo, h, n = FD.grid_from_bounds(w['bounds'], (1, 1, 1))
    V, rep = engine.cell_solid_volume(w['v'], w['f'], lo, h, n, report=True)
    assert rep['pairs'] == 5000 and rep['k_A'] == rep['k_P'] == 62 - 13                 # 5000 <= 2^13
    assert V.tobytes() == engine.cell_solid_volume(w['v'], w['f'], lo, h, n).tobytes()
    assert rel_err(V[0, 0, 0], w['volume'], tag='solid wire one cell closure') <= 1e-12
    H = FD.solid_volume(w['v'], w['f'], lo, h, n)
    cv = float(np.prod(h))
    print('wire one cell: |device - host| = %.3e cells' % (abs(V[0, 0, 0] - H[0, 0, 0]) / cv))
    assert allclose(V / cv, H / cv, rtol=0.0, atol=TOL_SOLID_WIRE, tag='solid wire one cell device against host (cells)')


def test_error_paths():
    from nanokappa_amd import engine, field as FD
    from nanokappa_amd.engine import NkError
    m, lo, h, n = case('cyl7', (5, 3, 2))
    with pytest.raises(NkError, match='at least one triangle'):
        engine.cell_solid_volume(m.vertices, m.faces[:0], lo, h, n)
    with pytest.raises(NkError, match='h must be positive'):
        engine.cell_solid_volume(m.vertices, m.faces, lo, h * np.array([1.0, 0.0, 1.0]), n)
    with pytest.raises(NkError, match='2\\^24 cells'):
        engine.cell_solid_volume(m.vertices, m.faces, lo, h, (257, 256, 256))
    with pytest.raises(NkError, match='does not contain the bounding box'):
        engine.cell_solid_volume(m.vertices, m.faces, lo + 0.5 * h, h, n)
    # ... and a valid call works afterwards
    V = engine.cell_solid_volume(m.vertices, m.faces, lo, h, n)
    assert rel_err(V.sum(), m.volume, tag='solid closure after errors') <= 1e-12
    assert engine.load_library().nk_solid_last_error() == b''


# ---------------------------------------------------------------------------------------------- Population
CYL_ARGV = ['--geometry', 'cylinder', '--dimensions', '500', '100', '16', '--subvolumes', 'slice', '10', '2',
            '--bound_pos', 'relative', '0.5', '0.5', '0', '0.5', '0.5', '1', '--bound_cond', 'T', 'T', 'R',
            '--bound_values', '302', '298', '5', '--poscar_file', 'POSCAR', '--hdf_file', 'synthetic',
            '--reference_temp', 'local', '--temp_dist', 'cold', '--temp_interp', 'linear', '--part_dist', 'random_subvol',
            '--timestep', '1', '--n_mean', '3', '--conv_crit', '0', '10', '--output', 'screen', '--energy_normal', 'fixed',
            '--particles', 'total', '50000', '--seed', '7', '--iterations', '60', '--field_grid', '6', '6', '4', '10']


def run_cylinder(folder, extra):
    """A parameter-file run of the 16-sided cylinder, 60 steps (windows of 30: n_mean 3 rows of 10 steps)."""
    from nanokappa_amd import nanokappa
    os.makedirs(str(folder), exist_ok=True)
    pf = os.path.join(str(folder), 'params.txt')
    with open(pf, 'w') as f:
        f.write(' '.join(CYL_ARGV + list(extra) + ['--results_folder', os.path.join(str(folder), 'run')]))
    cwd = os.getcwd()
    os.chdir(str(folder))
    try:
        return nanokappa.main(['-ff', pf])
    finally:
        sys.stdout = sys.__stdout__
        os.chdir(cwd)


def scalar_path(pop, raw, ref):
    """What Population.field() computed before it knew solid fractions: field.normalise with the whole cell's volume."""
    from nanokappa_amd import field as FD
    ph = pop._ph
    return FD.normalise(raw['N'], raw['E'], raw['F'], raw['samples'], ph.number_of_active_modes, ph.number_of_qpoints * ph.volume_unitcell,
                        pop.eVpsa2_in_Wm2, norm=pop.norm, particle_density=pop.particle_density, cell_volume=float(np.prod(pop.field_h)),
                        ref_energy=ref, temperature_function=ph.temperature_function if ref is not None else None)


def reference_energy(pop):
    """The reference energy Population.field() adds per cell (the subvolume of the cell's centre)."""
    from nanokappa_amd import field as FD
    cen = FD.cell_centres(pop.field_lo, pop.field_h, pop.field_n).reshape(-1, 3)
    sv = pop._geo.subvol_classifier.predict(cen)
    return np.asarray(pop._ph.crystal_energy_function(pop._window_T()))[sv].reshape(pop.field_n)


@pytest.fixture(scope='module')
def flagged(tmp_path_factory):
    """The run with --field_solid, once for the module: the population, its field() and the raw sums of the window it shows."""
    pop = run_cylinder(tmp_path_factory.mktemp('solid_on'), ['--field_solid'])
    assert pop._field_last is not None
    return dict(pop=pop, field=pop.field(), raw=pop._field_last)


# array cell volume against scalar / fraction: the same factors in another order, each operation within 2^-53 relative
TOL_NORM = 8 * 2.0 ** -53


def test_population_with_field_solid(flagged):
    from nanokappa_amd import engine, field as FD
    pop, f, raw = flagged['pop'], flagged['field'], flagged['raw']
    assert pop.norm == 'fixed' and f['n'] == (6, 6, 4) and f['samples'] == 3
    geo = pop._geo
    cv = float(np.prod(pop.field_h))
    V = engine.cell_solid_volume(geo.mesh.vertices, geo.mesh.faces, pop.field_lo, pop.field_h, pop.field_n)
    assert np.array_equal(f['solid_fraction'], V / cv)
    assert rel_err(V.sum(), geo.mesh.volume, tag='solid population closure') <= 1e-12
    fr = f['solid_fraction']
    assert fr.min() > 0.0 and fr.max() <= 1.0 + 1e-12 and (fr < 0.9).sum() >= 1          # every cell holds solid, some are cut
    assert 'N_outside' in f and f['N_outside'] == 0.0
    r = FD.read_vtk(FD.field_path(pop.results_folder_name))
    assert np.array_equal(r['solid_fraction'], fr)
    for k in ('N', 'T', 'energy', 'heat_flux'):
        assert np.array_equal(r[k], f[k], equal_nan=True), k
    # energy - ref and heat_flux: a second normalise call with the scalar cell volume, divided by the fraction
    a = scalar_path(pop, raw, None)
    ref = reference_energy(pop)
    want = a['energy'] / fr
    got = f['energy'] - ref
    # (adding ref and taking it off again costs 2^-53 of the sum each time)
    assert np.all(np.abs(got - want) <= TOL_NORM * np.abs(want) + 2.0 ** -52 * np.abs(f['energy']))
    want = a['heat_flux'] / fr[..., None]
    assert np.all(np.abs(f['heat_flux'] - want) <= TOL_NORM * np.abs(want))
    assert np.all(np.isfinite(f['T']))
    assert np.array_equal(f['N'], a['N'])


def test_population_without_field_solid(flagged, tmp_path):
    """The same run without the option: no solid_fraction anywhere, and N, T, energy, heat_flux are, to the byte, what the
    flagged run's raw sums give through the scalar path."""
    from nanokappa_amd import field as FD
    pop = run_cylinder(tmp_path / 'solid_off', [])
    f = pop.field()
    assert 'solid_fraction' not in f and 'N_outside' not in f and pop.field_solid_fraction is None
    path = FD.field_path(pop.results_folder_name)
    assert 'solid_fraction' not in FD.read_vtk(path) and b'solid_fraction' not in open(path, 'rb').read()
    fp = flagged['pop']
    old = scalar_path(fp, flagged['raw'], reference_energy(fp))
    assert f['samples'] == flagged['field']['samples']
    for k in ('N', 'T', 'energy', 'heat_flux'):
        assert f[k].tobytes() == old[k].tobytes(), k
    assert 'field_solid' not in open(os.path.join(pop.results_folder_name, 'arguments.txt')).read()
    assert '--field_solid\n' in open(os.path.join(fp.results_folder_name, 'arguments.txt')).read()
