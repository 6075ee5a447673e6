"""nk_reflect at its edges, through the tap (Engine.reflect): the diffuse pick through the bucket index against the
reference's search over the whole roulette row (reflect_cases.rule) on every entry, bucket edge and tie, with the index built
on the host (nk_set_rough) and on the device (k_rough_lut); and the specular branch at its two thresholds.  Modes are integers:
every comparison of them is an equality.  test_reflect_edges_host.py holds the oracle and the lattice to the same rule.
Needs a real MI355X: run with `pytest -m gpu`."""
import os
import sys

import numpy as np
import pytest

import reflect_cases as RC
from util import golden, golden_phonon, rel_err, TOL_OCC

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden'))


def engine_for(mc):
    from nanokappa_amd.engine import Engine
    eng = Engine(0, 3)
    eng.set_material(mc['tables'])
    eng.set_mesh(mc['mesh'])
    eng.set_subvolumes(mc['centers'], mc['volumes'], 0, mc['axis'], 1, mc['T_sv'])
    return eng


def diffuse_on_pair(eng, mc, names, pair, spec_tables, only=None):
    """The lattices of two rows, one per rough facet (only: of that facet's row alone), through nk_set_rough and the tap with
    r_spec = 2 (never specular)."""
    M = mc['M']
    sp, ts, sm = spec_tables
    roul = np.stack(pair)
    eng.set_rough(mc['facets'], sp, ts, sm, roul, None)
    lat = [RC.lattice(r) if only in (None, f) else np.zeros(0) for f, r in enumerate(pair)]
    facet, mode_in, col, n_in, om_in = RC.points(mc, lat)
    r_diff = np.concatenate(lat)
    r_spec = np.full(r_diff.shape[0], 2.0)
    mo, no, oo = eng.reflect(facet, mode_in, col, n_in, om_in, r_spec, None, r_diff)
    n0 = lat[0].shape[0]
    for name, row, la, got in ((names[0], pair[0], lat[0], mo[:n0]), (names[1], pair[1], lat[1], mo[n0:])):
        want = RC.rule(row, la)
        assert np.array_equal(got, want), RC.describe('%s M=%d' % (name, M), row, la, got, want)
    assert np.array_equal(oo, mc['tables']['omega'].ravel()[mo]), 'omega_out is not omega[mode_out]: %s' % (names,)
    _, no_o, _ = RC.oracle_reflect(mc, (sp, ts, sm, roul, None), facet, mode_in, col, n_in, om_in, r_spec, None, r_diff)
    e = rel_err(no, no_o, depth=2, tag='n_out M=%d' % M, bound=TOL_OCC)
    assert e < TOL_OCC, 'n_out differs from the oracle by %.3e: %s' % (e, names)
    return r_diff.shape[0]


@pytest.mark.parametrize('M', [4374, 162, 29478])
def test_diffuse_pick_with_the_host_built_index(M):
    """Every hand-made row (at 29478 modes: the three that need the size), and at 4374 modes the case's own four rows, on
    their full lattices: mode_out is np.searchsorted over the whole row, omega_out the picked mode's, n_out the oracle's.
    162 modes: almost every bucket is empty; 29478: a third index size (8192 buckets)."""
    mc = RC.material_case(M)
    rows = RC.rows(M)
    if M != 29478:
        names = sorted(rows)
        assert len(names) % 2 == 0
        jobs = [((a, b), None) for a, b in zip(names[0::2], names[1::2])]
    else:                                             # one row per call: the lattice of a row has 190 000 points
        c, p, r = RC.ROWS_29478
        jobs = [((c, p), 0), ((c, p), 1), ((r, c), 0)]
    eng = engine_for(mc)
    largest = 0
    for (a, b), only in jobs:
        largest = max(largest, diffuse_on_pair(eng, mc, (a, b), (rows[a], rows[b]), RC.never_specular(M), only))
    if M == 4374:
        for model in ('velocity', 'k'):
            r = RC.case_tables('ttrrp', model)['rough']
            diffuse_on_pair(eng, mc, (model + ' facet 0', model + ' facet 1'), (r['roulette'][0], r['roulette'][1]),
                            (r['specularity'], r['true_spec'], r['spec_map']))
    assert largest < 200000
    eng.close()


@pytest.mark.parametrize('model', ['velocity', 'k'])
def test_diffuse_pick_with_the_device_built_index(model):
    """The tables of the T T R R P box built on the device (k_rough_cumsum, k_rough_lut), as
    test_rough_tables_built_on_device_equal_host_builders_and_goldens builds them; the rule and the lattice on the roulette
    the device itself made (it may differ from the host's in the last bits).  The only check of k_rough_lut against the
    kernel that reads it at ties and bucket edges."""
    from nanokappa_amd import setup_tables as ST
    from nanokappa_amd.argument_parser import initialise_parser
    from nanokappa_amd.geometry import Geometry
    import ref_harness_args as A
    args = initialise_parser().parse_args(A.argv_for('ttrrp', 100000) + (['--bound_scat', 'k'] if model == 'k' else []))
    args.results_folder = ''
    geo = Geometry(args)
    ph = golden_phonon()
    mc = RC.material_case(4374)
    from nanokappa_amd.engine import Engine
    eng = Engine(0, 3)
    eng.set_material(ph.tables())
    eng.set_mesh(geo.tables())
    if model == 'k':
        # the reference's own choice among equally short images of zone-boundary q-points (test_gpu_parity.py)
        ph.wavevectors = golden('phonon')['wavevectors'].copy()
        deg, didx = ST.find_degeneracies(ph)
        ST.rough_tables_device_k(eng, geo, ph, geo.rough_facets, geo.rough_facets_values, deg, didx)
    else:
        ST.rough_tables_device(eng, geo, ph, geo.rough_facets, geo.rough_facets_values)
    eng.set_subvolumes(mc['centers'], mc['volumes'], 0, mc['axis'], 1, mc['T_sv'])
    sp, ts, sm, ro = eng.rough_download()
    assert ro.shape == (2, 4374) and np.all(np.isfinite(ro)) and np.all(np.diff(ro, axis=1) >= 0)
    assert np.array_equal(np.asarray(geo.rough_facets), mc['facets'])
    host = RC.case_tables('ttrrp', model)['rough']['roulette']
    assert np.allclose(ro, host, rtol=0, atol=1e-13)
    print('device-built roulette: %d of %d entries differ from the host-built one' % (int((ro != host).sum()), ro.size))
    lat = [RC.lattice(r) for r in ro]
    for f in (0, 1):
        assert RC.ties(ro[f], lat[f]).sum() >= 1900
    facet, mode_in, col, n_in, om_in = RC.points(mc, lat)
    r_diff = np.concatenate(lat)
    mo, no, oo = eng.reflect(facet, mode_in, col, n_in, om_in, np.full(r_diff.shape[0], 2.0), None, r_diff)
    n0 = lat[0].shape[0]
    for f, la, got in ((0, lat[0], mo[:n0]), (1, lat[1], mo[n0:])):
        want = RC.rule(ro[f], la)
        assert np.array_equal(got, want), RC.describe('%s facet %d, device-built' % (model, f), ro[f], la, got, want)
    assert np.array_equal(oo, ph.omega.ravel()[mo])
    eng.close()


@pytest.mark.parametrize('with_degen', [True, False])
def test_specular_threshold_and_degenerate_coin(with_degen):
    """r_spec <= specularity and r_deg >= 0.5 at equality and one double to either side, for specularities 0, 2^-53, 0.25,
    the last double below 1 and 1: mode_out by the reference's lines; a specular reflection keeps n and omega bit for bit; a
    diffuse one picks by the rule.  Without degen_j2 the coin is ignored."""
    mc = RC.material_case(4374)
    M, J = mc['M'], mc['J']
    sp, ts, sm, dj = RC.specular_tables(M, J)
    if not with_degen:
        dj = None
    roul = RC.case_tables('ttrrp', 'velocity')['rough']['roulette']
    f, m, r_spec, r_deg, r_diff = RC.specular_product(sp[0], [RC.lattice(roul[0]), RC.lattice(roul[1])])
    spec, want = RC.specular_rule(J, sp, ts, sm, dj, roul, f, m, r_spec, r_deg, r_diff)
    assert spec.sum() > 10000 and (~spec).sum() > 10000 and f.shape[0] < 200000
    _, _, col, n_in, om_in = RC.points(mc, [f])
    eng = engine_for(mc)
    eng.set_rough(mc['facets'], sp, ts, sm, roul, dj)
    mo, no, oo = eng.reflect(mc['facets'][f], m, col, n_in, om_in, r_spec, r_deg, r_diff)
    bad = np.nonzero(mo != want)[0]
    assert bad.shape[0] == 0, '%d differ; first: facet %d mode_in %d sp %s r_spec %s r_deg %s r_diff %s: got %d, expected %d' % (
        bad.shape[0], f[bad[0]], m[bad[0]], float.hex(float(sp[f[bad[0]], m[bad[0]]])), float.hex(float(r_spec[bad[0]])),
        float.hex(float(r_deg[bad[0]])), float.hex(float(r_diff[bad[0]])), mo[bad[0]], want[bad[0]])
    assert np.array_equal(no[spec], n_in[spec]) and np.array_equal(oo[spec], om_in[spec])
    for k in (0, 1):
        w = ~spec & (f == k)
        assert np.array_equal(mo[w], RC.rule(roul[k], r_diff[w]))
    assert np.array_equal(oo[~spec], mc['tables']['omega'].ravel()[mo[~spec]])
    _, no_o, _ = RC.oracle_reflect(mc, (sp, ts, sm, roul, dj), mc['facets'][f], m, col, n_in, om_in, r_spec, r_deg, r_diff)
    assert rel_err(no, no_o, tag='n_out', bound=TOL_OCC) < TOL_OCC
    eng.close()
