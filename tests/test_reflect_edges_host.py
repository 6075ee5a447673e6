"""Rough-wall reflection at its edges, the part that needs no GPU (reflect_cases.py): the oracle's nko_reflect, which the
multi-step parity tests trust, against np.searchsorted on every entry, bucket edge and tie and against the reference's lines at
the two thresholds of the specular branch; the bracketed search of nk_reflect restated in NumPy, right as it stands and
noticed by the lattice in each of four wrong variants; and the conditions on the inputs that keep these tests from running
empty."""
import numpy as np
import pytest

import reflect_cases as RC


def oracle_diffuse(mc, pair):
    """nko_reflect's picks with r_spec = 2 (never specular) on the lattices of two rows, one per rough facet."""
    lat = [RC.lattice(r) for r in pair]
    facet, mode_in, col, n_in, om_in = RC.points(mc, lat)
    r_diff = np.concatenate(lat)
    rough = RC.never_specular(mc['M']) + (np.stack(pair), None)
    mo, no, oo = RC.oracle_reflect(mc, rough, facet, mode_in, col, n_in, om_in, np.full(r_diff.shape[0], 2.0), None, r_diff)
    return lat, mo, oo


@pytest.mark.parametrize('M', [162, 4374])
def test_oracle_diffuse_pick_equals_searchsorted_on_hand_made_rows(M):
    mc = RC.material_case(M)
    rows = RC.rows(M)
    names = sorted(rows)
    for a, b in zip(names[0::2], names[1::2]):
        lat, mo, oo = oracle_diffuse(mc, (rows[a], rows[b]))
        n0 = lat[0].shape[0]
        for name, la, got in ((a, lat[0], mo[:n0]), (b, lat[1], mo[n0:])):
            want = RC.rule(rows[name], la)
            assert np.array_equal(got, want), RC.describe(name, rows[name], la, got, want)
        assert np.array_equal(oo, mc['tables']['omega'].ravel()[mo])
    assert len(names) % 2 == 0


@pytest.mark.parametrize('model', ['velocity', 'k'])
def test_oracle_diffuse_pick_equals_searchsorted_on_the_case_rows(model):
    mc = RC.material_case(4374)
    cr = RC.case_rows()
    pair = (cr[(model, 0)], cr[(model, 1)])
    lat, mo, _ = oracle_diffuse(mc, pair)
    n0 = lat[0].shape[0]
    for f, la, got in ((0, lat[0], mo[:n0]), (1, lat[1], mo[n0:])):
        want = RC.rule(pair[f], la)
        assert np.array_equal(got, want), RC.describe('%s facet %d' % (model, f), pair[f], la, got, want)


@pytest.mark.parametrize('with_degen', [True, False])
def test_oracle_specular_threshold_and_degenerate_coin(with_degen):
    mc = RC.material_case(4374)
    M, J = mc['M'], mc['J']
    sp, ts, sm, dj = RC.specular_tables(M, J)
    if not with_degen:
        dj = None
    roul = RC.case_tables('ttrrp', 'velocity')['rough']['roulette']
    f, m, r_spec, r_deg, r_diff = RC.specular_product(sp[0], [RC.lattice(roul[0]), RC.lattice(roul[1])])
    spec, want = RC.specular_rule(J, sp, ts, sm, dj, roul, f, m, r_spec, r_deg, r_diff)
    _, _, col, n_in, om_in = RC.points(mc, [f])
    mo, no, oo = RC.oracle_reflect(mc, (sp, ts, sm, roul, dj), mc['facets'][f], m, col, n_in, om_in, r_spec, r_deg, r_diff)
    assert np.array_equal(mo, want)
    assert np.array_equal(no[spec], n_in[spec]) and np.array_equal(oo[spec], om_in[spec])
    assert np.array_equal(oo[~spec], mc['tables']['omega'].ravel()[mo[~spec]])
    # the product reaches what it is for: both sides of both thresholds, and equality at each
    assert spec.sum() > 10000 and (~spec & ts[f, m].astype(bool)).sum() > 10000
    assert (ts[f, m].astype(bool) & (r_spec == sp[f, m])).sum() > 10000 and (r_deg == 0.5).sum() > 10000
    if with_degen:
        coin = spec & (dj[sm[f, m] * spec] > -1)
        assert (coin & (r_deg >= 0.5)).sum() > 1000 and (coin & (r_deg < 0.5)).sum() > 1000
        assert np.any(want[coin & (r_deg >= 0.5)] != sm[f, m][coin & (r_deg >= 0.5)])


def all_rows():
    out = [('%s facet %d' % k, r) for k, r in sorted(RC.case_rows().items())]
    for M in (162, 4374):
        out += [('%s M=%d' % (k, M), r) for k, r in sorted(RC.rows(M).items())]
    out += [('%s M=29478' % k, RC.rows(29478)[k]) for k in RC.ROWS_29478]
    return out


def test_bracketed_search_equals_the_rule_everywhere():
    """Index plus search inside the bracket, as nk_reflect does it with the index of nk_set_rough / k_rough_lut, is the
    full-table search on every table and lattice used here: a failure of the GPU tests is the kernel's."""
    for name, row in all_rows():
        la = RC.lattice(row)
        got, want = RC.bracketed(row, la), RC.rule(row, la)
        assert np.array_equal(got, want), RC.describe(name, row, la, got, want)


def test_lattice_notices_each_wrong_variant():
    """Four mistakes an edit of the kernel or of an index builder could make, each seen by the lattice; the index built with a
    right search shows on one point of a case row and on a clustered hand-made row."""
    cr = RC.case_rows()
    seen = {}
    for v in RC.VARIANTS:
        for key, row in sorted(cr.items()):
            la = RC.lattice(row)
            n = int(np.sum(RC.bracketed(row, la, v) != RC.rule(row, la)))
            seen[(v,) + key] = n
            if v != 'index_right':
                assert n > 0, (v, key)
    print(seen)
    assert seen[('inner_le', 'velocity', 0)] >= 1900
    assert seen[('bucket_rounded', 'velocity', 0)] >= 3000 and seen[('at_most_four', 'velocity', 0)] >= 2000
    row = RC.rows(4374)['cluster']
    la = RC.lattice(row)
    n = int(np.sum(RC.bracketed(row, la, 'index_right') != RC.rule(row, la)))
    print('index_right on cluster:', n)
    assert n > 0
    assert sum(seen[('index_right',) + k] for k in cr) > 0


def test_conditions_on_the_inputs():
    """What the tests above and on the GPU rely on, so that a change of tables cannot quietly empty them."""
    for key, row in sorted(RC.case_rows().items()):
        la = RC.lattice(row)
        kb, lo, hi = RC.brackets(row, la)
        print(key, la.shape[0], int(RC.ties(row, la).sum()), int((hi - lo > 4).sum()))
        assert row.shape[0] == 4374 and RC.nlut_of(row.shape[0]) == 2048
        assert la.shape[0] == 20136
        assert RC.ties(row, la).sum() >= 1900
        assert (hi - lo > 4).sum() >= 5000
        assert la[0] == 0.0 and la[1] == 5e-324 and la[-1] == np.nextafter(1.0, 0.0) and np.all(np.diff(la) > 0)
    big = RC.rows(4374)
    for name in ('step', 'cluster'):
        la = RC.lattice(big[name])
        kb, lo, hi = RC.brackets(big[name], la)
        assert (hi - lo > 4).sum() > 0, name
    assert RC.rule(big['step'], np.zeros(1))[0] == 0                 # r_diff = 0 on a row that starts with zeros: mode 0
    kb, lo, hi = RC.brackets(big['step'], np.zeros(1))
    assert hi[0] - lo[0] > 2000
    small = RC.rows(162)
    for name, row in small.items():
        lut = RC.build_index(row, RC.nlut_of(162))
        assert (np.diff(lut) == 0).sum() > 1024 // 2, name
    for M in (162, 4374, 29478):
        for name in RC.LAST_NOT_ONE:
            row = RC.rows(M)[name]
            assert row[-1] != 1.0 and RC.ties(row, RC.lattice(row)).sum() > 0, (M, name)
    # the lattice is what reflect_cases says: entries, edges, and their neighbours
    row = RC.rows(162)['ramp*0.7']
    la = RC.lattice(row)
    for base in (np.unique(row / row[-1]), np.arange(1025) / 1024.0):
        for s in (0, 1, 2, -1, -2):
            p = RC._moved(base, s)
            assert np.all(np.isin(p[(p >= 0) & (p < 1)], la))
