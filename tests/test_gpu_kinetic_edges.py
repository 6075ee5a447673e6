"""Kinetic flights on the GPU at their edges (tests/kinetic_edge_cases.py; k_kinetic<GEOM, BINS, GROUPED>, k_kinetic_fold, nk_kin_run)
against the CPU restatement: rays that end as lost or capped, terms above their bounds that are left out of the integer sums and
counted, modes that sit, specular turns into modes that do not live, six and eight sources, launch shapes that leave lanes idle,
bins that do not fit the LDS, and the grouped instantiations on the same inputs.

What is compared how:
  * the discrete outputs -- start points, modes, ends, event and cast counts, event hashes, the ends matrix, the counts of lost,
    missed and capped rays and every left-out count by source (rows[:, 20:25]) -- bit for bit;
  * a ray's displacement absolutely and its dwell time relatively, within <= 10 x the largest deviation measured on an MI355X for
    that case (profiles/kinetic_margins.txt; the device logarithm's last bit and one rounding per segment): TOL_D, TOL_DWELL;
  * the integer sums `rows` against the host's sums of the engine's OWN per-ray outputs with the same bounds (a term above its
    bound adds 0 and is counted once), bit for bit; `sub` (and `grp`) against the restatement's: the same nonzero pattern and at
    most one unit per segment, the rule of test_gpu_kinetic.py.
Every case's rays keep their event sequence between fused and unfused positions on the CPU (test_kinetic_edges_host.py), so no
ray is left out of a comparison."""
import re

import numpy as np
import pytest

import kinetic_cases as K
import kinetic_edge_cases as E
import free_path_cases as FC
from nanokappa_amd import kinetic as KN
from util import allclose, rel_err

pytestmark = pytest.mark.gpu

# angstrom / relative, per case: <= 10 x the deviation measured on an MI355X (profiles/kinetic_margins.txt, "kinetic edges").  0: the
# kernel gave the restatement's bits and the test asks for them -- 'all_lost' has no segment, 'leftout_ray' is ballistic (every t
# is a cast's, no logarithm), the dwell times of 'capped_5' and 'some_lost' happened to.  'some_lost' holds rays that fly 1024
# segments nearly along the walls, tens of thousands of angstrom sideways; 'stationary' and its like end segments at a wall in slow
# modes, where one ulp of the position (2.8e-14 A) is 1e-14 ps of flight.
TOL_D = {'all_lost': 0.0, 'some_lost': 7e-11, 'capped_1': 3.5e-14, 'capped_2': 1.4e-13, 'capped_5': 1.4e-13, 'stationary': 2.2e-12,
         'dead_turn': 5e-13, 'leftout_segment': 3.5e-14, 'leftout_ray': 0.0, 'six_sources': 7e-14, 'eight_sources': 2.4e-12,
         'bins_do_not_fit': 2.8e-13, 'shapes': 1e-12, 'shapes_1': 3.5e-14}          # ('shapes_1': the shapes with a single ray per source)
TOL_DWELL = {'all_lost': 0.0, 'some_lost': 0.0, 'capped_1': 2.4e-15, 'capped_2': 2.9e-15, 'capped_5': 0.0, 'stationary': 5.9e-14,
             'dead_turn': 3.7e-15, 'leftout_segment': 1.9e-15, 'leftout_ray': 0.0, 'six_sources': 1.3e-15, 'eight_sources': 1.6e-14,
             'bins_do_not_fit': 3.8e-15, 'shapes': 1.8e-15, 'shapes_1': 1.3e-15}
ENGINE_OF = {'dead_turn': 'spec1', 'leftout_segment': 'spec1', 'six_sources': 'six', 'eight_sources': 'eight', 'bins_do_not_fit': 'box128'}
RAY_KEYS = ('ray_x0', 'ray_mode', 'ray_end', 'ray_events', 'ray_casts', 'ray_D', 'ray_dwell', 'ray_hash')
ALL_KEYS = ('rows', 'sub', 'ends', 'lost', 'missed', 'capped', 'events', 'casts', 'D', 'D2', 'dwell_total', 'dwell', 'flux') + RAY_KEYS
_ENG = {}


def engine(name):
    """One engine per set of tables for the whole module: the cases on the unchanged 'ttp' tables share theirs."""
    from test_gpu_free_path import fp_engine
    key = ENGINE_OF.get(name, 'ttp')
    if key not in _ENG:
        _ENG[key] = fp_engine(E.inputs(name)['ct'] if key != 'ttp' else K.case('ttp'), seed=99)
    return _ENG[key]


def call(name, monkeypatch, **kw):
    """Engine.kinetic_flights on a case's inputs with rays=True (kw: rays_per_wave, lds_bins, groups)."""
    inp = E.inputs(name)
    if inp['tables'] is not None:
        monkeypatch.setattr(KN, 'tables', inp['tables'])
    return engine(name).kinetic_flights(inp['tau'], inp['c'], n=inp['n'], seed=inp['seed'], max_events=inp['max_events'], rays=True, **kw)


def plain(name, monkeypatch):
    """The case's call with the defaults, made once."""
    return FC.cached(('kin_edge_gpu', name), lambda: call(name, monkeypatch))


def assert_words(got, want, events, what):
    d = np.abs(np.asarray(got, dtype=np.int64) - want)
    print('%s: largest |difference| of a word %d (events %d)' % (what, d.max() if d.size else 0, events))
    assert np.array_equal(got != 0, want != 0), what
    assert d.max() <= events, what


def compare(name, got, ref, tol=''):
    """A call against the restatement of the same inputs: the module docstring's three rules."""
    rep = got['report']
    for k in ('ray_x0', 'ray_mode', 'ray_end', 'ray_events', 'ray_casts', 'ray_hash', 'ends', 'lost', 'missed', 'capped', 'events', 'casts'):
        assert np.array_equal(got[k], ref[k]), (name, k)
    assert np.array_equal(got['rows'][:, 20:25], ref['rows'][:, 20:25]), (got['rows'][:, 20:25], ref['rows'][:, 20:25])
    for k in ('k_t', 'k_x', 'k_T', 'k_D', 'k_D2', 'B_t', 'B_x', 'lost', 'missed', 'capped', 'events', 'casts', 'overflow'):
        assert rep[k] == ref['report'][k], (name, k)
    tol = tol or name
    ok_D = allclose(got['ray_D'], ref['ray_D'], rtol=0, atol=TOL_D[tol], tag=name + ' D')
    worst = rel_err(got['ray_dwell'], ref['ray_dwell'], tag=name + ' dwell', bound=TOL_DWELL[tol])
    assert ok_D, 'displacements differ'
    assert worst <= TOL_DWELL[tol]
    assert np.array_equal(got['rows'], E.host_rows(got)), name
    assert rep['overflow'] == got['rows'][:, 20:25].sum()
    assert_words(got['sub'], ref['sub'], rep['events'], name + ' sub')


def counts_in(message):
    """The five counts an overflow text names, in the order of rows[:, 20:25]."""
    m = re.search(r'overflow: (\d+) displacement\(s\), (\d+) squared displacement\(s\) and (\d+) dwell time\(s\) of a ray, (\d+) time\(s\) and '
                  r'(\d+) displacement\(s\) of a segment above their bounds; they were left out of the sums', message)
    assert m, message
    return [int(x) for x in m.groups()]


@pytest.mark.parametrize('name', sorted(E.CASES))
def test_case_against_restatement(name, monkeypatch):
    got, ref = plain(name, monkeypatch), E.run(name)
    rep = got['report']
    print('%s: %d rays, %d events, lost %d, missed %d, capped %d, left out %s' % (name, rep['rays'], rep['events'], rep['lost'], rep['missed'],
                                                                                rep['capped'], got['rows'][:, 20:25].sum(axis=0).tolist()))
    compare(name, got, ref)
    assert (rep['message'] == '') == (rep['overflow'] == 0)
    if name == 'all_lost':
        assert not got['rows'][:, :8].any() and not got['rows'][:, 11:].any() and not got['sub'].any() and np.array_equal(got['lost'], [256, 256])
    if name == 'leftout_ray':
        assert not got['sub'].any() and not got['rows'][:, 13:19].any() and (got['rows'][:, 19] > 0).all() and (got['rows'][:, 20:25] > 0).all()
    if name == 'eight_sources':
        assert rep['geometry_mode'] == 2 and rep['n_sources'] == 8 and rep['source_facet'] == list(E.EIGHT_SOURCES)
    if name == 'bins_do_not_fit':
        assert rep['lds_bins'] == 0 and rep['n_sources'] == 6 and rep['n_subvolumes'] == 128             # without being asked
    else:
        assert rep['lds_bins'] == 1


@pytest.mark.parametrize('name', E.LEAVES_OUT + ('some_lost',))
def test_leaving_terms_out(name, monkeypatch):
    """The call returns its results and says what it left out; the engine's next call is an ordinary one."""
    p = K.PARITY['ttp_16' if name != 'leftout_segment' else 'ttrrp_k']
    ct = K.case(p['case'])
    ordinary = lambda: engine(name).kinetic_flights(K.lifetimes(ct, p['scale']), K.heat_capacity(ct), n=64, seed=p['seed'], rays=True)
    before = ordinary()
    inp = E.inputs(name)
    if inp['tables'] is not None:
        monkeypatch.setattr(KN, 'tables', inp['tables'])
    got = engine(name).kinetic_flights(inp['tau'], inp['c'], n=inp['n'], seed=inp['seed'], max_events=inp['max_events'], rays=True)
    monkeypatch.undo()
    left = got['rows'][:, 20:25]
    assert got['report']['overflow'] == left.sum() > 0 and np.array_equal(left, E.run(name)['rows'][:, 20:25])
    assert counts_in(got['report']['message']) == left.sum(axis=0).tolist()
    if name in E.LEAVES_OUT:
        assert np.count_nonzero(left.sum(axis=0)) == (5 if name == 'leftout_ray' else 2)
    for k in ALL_KEYS:
        assert np.array_equal(got[k], plain(name, monkeypatch)[k]), k
    after = ordinary()
    assert after['report']['overflow'] == 0 and after['report']['message'] == '' and before['report']['message'] == ''
    for k in ALL_KEYS:
        assert np.array_equal(after[k], before[k]), k


@pytest.mark.parametrize('name', E.THREE_WAYS)
def test_three_ways(name, monkeypatch):
    a = plain(name, monkeypatch)
    g = call(name, monkeypatch, rays_per_wave=64)
    m = call(name, monkeypatch, lds_bins=False)
    F, n = a['ends'].shape[0], E.inputs(name)['n']
    assert a['report']['grid'] == -(-F // 4) and g['report']['grid'] == -(-(F * -(-n // 64)) // 4)
    assert a['report']['lds_bins'] == 1 and g['report']['lds_bins'] == 1 and m['report']['lds_bins'] == 0
    for k in ALL_KEYS:
        assert np.array_equal(a[k], g[k]) and np.array_equal(a[k], m[k]), k
    assert a['report']['message'] == g['report']['message'] == m['report']['message']


@pytest.mark.parametrize('name', E.GROUPED)
def test_groups(name, monkeypatch):
    a, ref = plain(name, monkeypatch), E.run_grouped(name)
    table = E.group_table(E.inputs(name)['tau'].shape[0])
    got = call(name, monkeypatch, groups=(3, table))
    assert got['grp'].shape == a['sub'].shape[:2] + (4, 4) and np.array_equal(got['grp'].sum(axis=2), got['sub'])
    for k in ALL_KEYS:
        assert np.array_equal(got[k], a[k]), k
    for k in ('overflow', 'message', 'events', 'casts', 'lost', 'missed', 'capped', 'k_t', 'k_x', 'B_t', 'B_x', 'grid'):
        assert got['report'][k] == a['report'][k], k
    assert np.array_equal(got['ray_hash'], ref['ray_hash'])
    assert_words(got['grp'], ref['grp'], got['report']['events'], name + ' group words')
    if name == 'leftout_ray':
        assert not got['grp'].any()
    if name == 'leftout_segment':
        # the modes reached by specular turns only, which cdf_scatter never draws, in a column of their own
        from test_kinetic_edges_host import partner_words
        want = partner_words()
        one = call(name, monkeypatch, groups=(1, E.partner_table(E.inputs(name))))
        assert one['grp'][:, :, 0].any() and np.array_equal(one['grp'].sum(axis=2), a['sub'])
        assert np.array_equal(one['grp'][:, :, 0] != 0, want[:, :, 0] != 0)
        assert_words(one['grp'], want, one['report']['events'], 'partner words')
        m = call(name, monkeypatch, groups=(3, table), lds_bins=False, rays_per_wave=64)
        assert np.array_equal(m['grp'], got['grp']) and np.array_equal(m['rows'], got['rows'])


@pytest.mark.parametrize('n,rays_per_wave', E.SHAPES)
def test_shapes(n, rays_per_wave):
    """A single ray, a last wave with one ray, blocks that are no multiple of 64 rays, one ray per wave."""
    p = K.PARITY['ttp_16']
    ct = K.case('ttp')
    tau, c = K.lifetimes(ct, p['scale']), K.heat_capacity(ct)
    full = FC.cached(('kin_edge_gpu_full',), lambda: engine('shapes').kinetic_flights(tau, c, n=K.PARITY_N, seed=p['seed'], rays=True))
    got = engine('shapes').kinetic_flights(tau, c, n=n, seed=p['seed'], rays=True, rays_per_wave=rays_per_wave)
    rpw = rays_per_wave or 512
    assert got['report']['grid'] == -(-(2 * -(-n // rpw)) // 4) and got['report']['rays'] == 2 * n and got['report']['overflow'] == 0
    for k in RAY_KEYS:
        assert got[k].shape[:2] == (2, n) and np.array_equal(got[k], full[k][:, :n]), k
    compare('shapes n=%d' % n, got, E.shape_run(n), tol='shapes_1' if n == 1 else 'shapes')
