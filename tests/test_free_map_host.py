"""Free-path maps without a GPU: the host functions of nanokappa_amd/free_map.py -- the integer tally that the GPU is held to
(tests/test_gpu_free_map.py), the scales, the two normalisations, the closed form averaged over a slab cell, the files and the
option -- and, end to end, the CPU restatement of the flight (tests/free_path_cases.py) tallied and normalised against the closed
form, which is the check that the reference rule alone stays inside the bound the GPU test uses."""
import numpy as np
import pytest

import free_path_cases as FC
from nanokappa_amd import field as FD
from nanokappa_amd import free_map as FM
from nanokappa_amd import free_path as FP

L_BOX = 200.0


# ------------------------------------------------------------------------------------------- shared with the GPU tests
def case_weights(ct, modes, T=FC.T_CASE):
    """(C [L], w [L, 3]) of a list of modes of a case: free_map.weights with the case's tables."""
    tb = ct['tables']
    C = FP.mode_heat_capacity(np.asarray(tb['omega'], dtype=float).ravel()[modes], T, tb['hbar'], tb['kb'])
    return C, FM.weights(C, FC.group_vel(ct)[modes], tb['QV'])


def profile_with_errors(x0, D, w, lo, h, n, kind, cell_fraction=None):
    """kappa_xx per cell in units of `unit` (sum of w_x D_x over a cell's rays, normalised) and its standard error, from per-ray
    terms x0, D [L, ns, 3] and weights w [L, 3].  The rays of a mode are independent draws, the modes are strata: with y = w_x
    D_x 1[x0 in c] and z = 1[x0 in c] per ray,
      'solid': sum y / (ns f_c), f_c the cell's share of the solid; variance sum_m ns var_m(y) / (ns f_c)^2;
      'count': L sum y / sum z, a ratio R = A / B; variance by linearisation, L^2 sum_m ns var_m(y - (A / B) z) / B^2.
    var_m is the sample variance over the ns rays of mode m (ns - 1 in the denominator)."""
    L, ns = D.shape[:2]
    c, _ = FD.cell_index(x0.reshape(-1, 3), lo, h, n)
    q = ((c[:, 0] * n[1] + c[:, 1]) * n[2] + c[:, 2]).reshape(L, ns)
    t = w[:, None, 0] * D[:, :, 0]
    nc = n[0] * n[1] * n[2]
    val, se = np.full(nc, np.nan), np.full(nc, np.nan)
    for cell in range(nc):
        z = (q == cell).astype(np.float64)
        y = t * z
        A, B = y.sum(), z.sum()
        if kind == 'solid':
            f = float(np.ravel(cell_fraction)[cell])
            val[cell] = A / (ns * f)
            se[cell] = np.sqrt((ns * y.var(axis=1, ddof=1)).sum()) / (ns * f)
        elif B > 0:
            val[cell] = L * A / B
            se[cell] = L * np.sqrt((ns * (y - (A / B) * z).var(axis=1, ddof=1)).sum()) / B
    return val.reshape(n), se.reshape(n)


def closed_form_profile(ct, modes, w, n_x, lo_x=0.0):
    """The closed form's kappa_xx(cell) / kappa_bulk,xx on n_x slab cells of the 'ttp' box, and kappa_bulk,xx in units of `unit`."""
    lam = FC.group_vel(ct)[modes, 0] * FC.lifetimes(ct)[modes]
    edges = np.linspace(0.0, L_BOX, n_x + 1)
    return FM.film_profile(w[:, 0], lam, L_BOX, edges[:-1], edges[1:]), float((w[:, 0] * lam).sum())


# ------------------------------------------------------------------------------------------- tally
GRID = (np.zeros(3), np.ones(3), (2, 1, 1))


def one_ray(x, D=(0.0, 0.0, 0.0), T=0.0, rw=0.0, end=3, w=(1.0, 1.0, 1.0), k=(0, 0, 0)):
    lo, h, n = GRID
    return FM.tally(np.array([[x, 0.5, 0.5]]), np.array([D]), [T], [rw], [end], np.array([w]), lo, h, n, *k)


def test_tally_cell_rule():
    """A ray on a cell border goes to the upper cell; a ray outside the grid (or a NaN) is clamped into the edge cell and the
    host counts it (field.cell_index)."""
    assert one_ray(1.0)[:, 0, 0, 0].tolist() == [0, 1]
    assert one_ray(np.nextafter(1.0, 0.0))[:, 0, 0, 0].tolist() == [1, 0]
    assert one_ray(-0.5)[:, 0, 0, 0].tolist() == [1, 0] and one_ray(7.0)[:, 0, 0, 0].tolist() == [0, 1]
    assert one_ray(np.nan)[:, 0, 0, 0].tolist() == [1, 0]
    lo, h, n = GRID
    _, out = FD.cell_index(np.array([[-0.5, 0.5, 0.5], [0.5, 0.5, 0.5], [7.0, 0.5, 0.5], [np.nan, 0.5, 0.5], [2.0, 0.5, 0.5]]), lo, h, n)
    assert out.tolist() == [True, False, True, True, True]


def test_tally_words_rounding_and_zero_terms():
    """Word 1 + 3a + b holds w_a D_b; the weight goes to word 10, 11 or 12 by the end code; ties round to even; a zero term
    leaves no trace and words 14, 15 stay zero."""
    c = one_ray(0.5, D=(1.0, 2.0, 3.0), T=5.0, rw=0.25, end=1, w=(10.0, 100.0, 1000.0), k=(0, 2, 1))[0, 0, 0]
    assert c.tolist() == [1, 10, 20, 30, 100, 200, 300, 1000, 2000, 3000, 1, 0, 0, 10, 0, 0]
    for end, word in ((1, 10), (2, 11), (4, 12), (0, 12)):
        c = one_ray(0.5, rw=0.5, end=end, k=(0, 1, 0))[0, 0, 0]
        assert c[word] == 1 and c[10:13].sum() == 1
    assert one_ray(0.5, rw=0.0, end=3, k=(0, 1, 0))[0, 0, 0, 10:13].tolist() == [0, 0, 0]          # a miss routes nothing
    # ties to even, both signs (k = 0: the terms are the integers' halves)
    for d, q in ((0.5, 0), (1.5, 2), (2.5, 2), (3.5, 4), (-0.5, 0), (-1.5, -2), (-2.5, -2), (2.5000000000000004, 3)):
        assert one_ray(0.5, D=(d, 0.0, 0.0), w=(1.0, 0.0, 0.0))[0, 0, 0, 1] == q, d
    assert one_ray(0.5, T=2.5)[0, 0, 0, 13] == 2 and one_ray(0.5, rw=1.5, end=2)[0, 0, 0, 11] == 2
    z = one_ray(0.5)
    assert z[0, 0, 0].tolist() == [1] + [0] * 15 and not z[1].any()
    neg = one_ray(0.5, D=(-3.0, 0.0, 0.0), w=(1.0, 0.0, 0.0))
    assert neg[0, 0, 0, 1] == -3 and neg.dtype == np.int64                                        # two's complement


def random_rays(rng, R):
    x0 = rng.uniform(-0.2, 2.2, (R, 3)) * np.array([1.0, 0.5, 0.5])
    D = rng.normal(0, 50.0, (R, 3))
    T = rng.uniform(0, 30.0, R)
    end = rng.integers(0, 5, R)
    rw = np.where(end == 3, 0.0, rng.uniform(0, 1, R))
    w = rng.normal(0, 1e-3, (R, 3))
    return x0, D, T, rw, end, w


def test_tally_commutes():
    """A permutation of the rays gives identical bytes; tally(A) + tally(B) == tally(A u B) at equal scales."""
    rng = np.random.default_rng(4)
    x0, D, T, rw, end, w = random_rays(rng, 3000)
    lo, h, n = np.zeros(3), np.array([0.5, 0.25, 0.5]), (4, 2, 1)
    k = (30, 40, 35)
    a = FM.tally(x0, D, T, rw, end, w, lo, h, n, *k)
    p = rng.permutation(3000)
    assert FM.tally(x0[p], D[p], T[p], rw[p], end[p], w[p], lo, h, n, *k).tobytes() == a.tobytes()
    A, B = p[:1234], p[1234:]
    ab = FM.tally(x0[A], D[A], T[A], rw[A], end[A], w[A], lo, h, n, *k) + FM.tally(x0[B], D[B], T[B], rw[B], end[B], w[B], lo, h, n, *k)
    assert np.array_equal(ab, a) and a[..., 0].sum() == 3000 and not a[..., 14:].any()
    # the integers stand for the float sums to within half a unit per ray
    c, _ = FD.cell_index(x0, lo, h, n)
    sel = (c == np.array([1, 0, 0])).all(axis=1)
    assert abs(np.ldexp(float(a[1, 0, 0, 1 + 3 * 2 + 1]), -30) - (w[sel, 2] * D[sel, 1]).sum()) <= sel.sum() * 2.0 ** -31 + 1e-12


def test_scales():
    """2^61 <= cap B 2^k <= 2^62 for the three sums (nk_field_k: one bit of headroom at most), monotone in capacity, floors
    respected."""
    rng = np.random.default_rng(7)
    v, tau = rng.normal(0, 40.0, (50, 3)), rng.uniform(-1.0, 300.0, 50)
    w = rng.normal(0, 1e-4, (10, 3))
    last = None
    for cap in (0, 1, 640, 641, 10 ** 6, 10 ** 9, 2 ** 40):
        s = FM.scales(w, v, tau, 640, capacity=cap)
        assert s['cap'] == max(640, cap)
        live = tau > 0
        assert s['B_T'] == tau[live].max() and s['B_K'] == np.abs(w).max() * (np.abs(v[live]).max(axis=1) * tau[live]).max()
        for B, k in ((s['B_K'], s['k_K']), (1.0, s['k_P']), (s['B_T'], s['k_T'])):
            assert 2.0 ** 61 <= np.ldexp(s['cap'] * B, k) <= 2.0 ** 62
        if last is not None:
            assert all(s[key] <= last[key] for key in ('k_K', 'k_P', 'k_T'))
        last = s
    big = FM.scales(w, v, tau, 640, weight_bound=1.0)
    assert big['B_K'] > s['B_K'] * 100 and big['k_K'] < FM.scales(w, v, tau, 640)['k_K']
    assert FM.scales(w, v, tau, 640, weight_bound=1e-9) == FM.scales(w, v, tau, 640)             # a floor below the maximum
    dead = FM.scales(w, v, -np.ones(50), 640)
    assert dead['B_K'] == 0.0 and dead['B_T'] == 0.0 and dead['k_K'] == 62


def test_normalise_on_synthetic_integers():
    """Both kinds on hand-made integers; empty cells NaN; 'solid' sums back to the global tensor."""
    n = (2, 2, 1)
    rep = dict(k_K=10, k_P=8, k_T=4)
    cells = np.zeros(n + (16,), dtype=np.int64)
    cells[0, 0, 0] = [40] + [int(x * 1024) for x in (1, 2, 3, 4, 5, 6, 7, 8, 9)] + [10 * 256, 20 * 256, 2 * 256, 80 * 16, 0, 0]
    cells[1, 0, 0] = [10] + [-1024] * 9 + [256, 0, 0, 16, 0, 0]
    cells[0, 1, 0] = [30] + [512] * 9 + [0, 0, 0, 0, 0, 0]                       # (a cell outside the solid that caught rays)
    n_list, ns = 5, 16
    m = FM.normalise(cells, rep, ns, n_list, 'count', unit=2.0, kappa_bulk=np.eye(3) * 4.0, axis=1)
    assert np.array_equal(m['kappa'][0, 0, 0], 2.0 * np.arange(1.0, 10.0).reshape(3, 3) / (40 / 5))
    assert np.array_equal(m['kappa'][1, 0, 0], np.full((3, 3), -2.0 / 2.0)) and np.isnan(m['kappa'][1, 1, 0]).all()
    assert m['suppression'][0, 0, 0] == m['kappa'][0, 0, 0, 1, 1] / 4.0 and np.isnan(m['suppression'][1, 1, 0])
    assert m['N'].tolist() == [[[40.0], [30.0]], [[10.0], [0.0]]]
    assert (m['p_res'][0, 0, 0], m['p_wall'][0, 0, 0], m['w_left'][0, 0, 0], m['p_int'][0, 0, 0]) == (0.25, 0.5, 0.05, 1 - 0.25 - 0.5 - 0.05)
    assert m['T_mean'][0, 0, 0] == 2.0 and m['T_mean'][1, 0, 0] == 0.1 and np.isnan(m['p_res'][1, 1, 0]) and np.isnan(m['T_mean'][1, 1, 0])
    assert np.isnan(FM.normalise(cells, rep, ns, n_list, 'count')['suppression']).all()             # no bulk value: no ratio
    fr = np.array([[[1.0], [0.0]], [[0.25], [5e-13]]])
    s = FM.normalise(cells, rep, ns, n_list, 'solid', solid_fraction=fr, cell_volume=8.0, unit=2.0, kappa_bulk=np.eye(3))
    assert np.isnan(s['kappa'][0, 1, 0]).all() and np.isnan(s['kappa'][1, 1, 0]).all()              # fractions <= SOLID_EMPTY
    assert np.array_equal(s['kappa'][0, 0, 0], 2.0 * np.arange(1.0, 10.0).reshape(3, 3) / (16 * 8.0 / 10.0))
    assert np.array_equal(s['kappa'][1, 0, 0], np.full((3, 3), -2.0 / (16 * 2.0 / 10.0)))
    # sum_c kappa(c) V_c / V = unit sum_c S(c) / n_samples over the cells in the solid: the global tensor of those rays
    S = FM.sums(cells, rep)['S']
    assert np.allclose(FM.solid_mean(s['kappa'], fr), 2.0 * (S[0, 0, 0] + S[1, 0, 0]) / ns, rtol=1e-15, atol=0)
    with pytest.raises(ValueError, match='solid'):
        FM.normalise(cells, rep, ns, n_list, 'solid')
    with pytest.raises(ValueError, match='kind'):
        FM.normalise(cells, rep, ns, n_list, 'mean')


def point_suppression(lam, x0):
    """D_x / Lambda_x of a ray from x0: 1 - exp(-d / |Lambda_x|), d the distance to the wall ahead."""
    d = np.where(lam > 0, L_BOX - x0, x0)
    return -np.expm1(-d / np.abs(lam))


def test_film_cell_suppression():
    """Against numerical quadrature over the cell to 1e-12 relative, and its volume mean against free_path.film_suppression.
    The integrand is the pointwise displacement whose mean over a whole slab of length d is free_path.film_displacement(v, tau,
    d) -- checked first, so the quadrature is anchored on that function; then the same integrand over one cell."""
    xg, wg = np.polynomial.legendre.leggauss(96)
    lams = np.array([2.0, 9.5, 40.0, 333.0, 5e3, 1e6, -2.0, -70.0, -2e4])
    # the anchor: the mean of the pointwise form over [0, L] is film_displacement / Lambda = film_suppression
    for lam in lams:
        sub = np.linspace(0.0, L_BOX, 41)                           # composite rule: 40 panels (the integrand decays over |lam|)
        tot = sum(0.5 * (b - a) * (wg * point_suppression(lam, 0.5 * (a + b) + 0.5 * (b - a) * xg)).sum() for a, b in zip(sub[:-1], sub[1:]))
        ref = FP.film_displacement(lam, 1.0, L_BOX) / lam
        assert abs(tot / L_BOX - ref) <= 1e-11 * ref, lam           # (film_suppression itself cancels for long paths)
    for n_x in (1, 4, 8, 5):
        edges = np.linspace(0.0, L_BOX, n_x + 1)
        got = FM.film_cell_suppression(lams[:, None], L_BOX, edges[None, :-1], edges[None, 1:])
        for i, lam in enumerate(lams):
            for c in range(n_x):
                a, b = edges[c], edges[c + 1]
                sub = np.linspace(a, b, 11)
                q = sum(0.5 * (v - u) * (wg * point_suppression(lam, 0.5 * (u + v) + 0.5 * (v - u) * xg)).sum() for u, v in zip(sub[:-1], sub[1:])) / (b - a)
                assert abs(got[i, c] - q) <= 1e-12 * q, (lam, n_x, c)
        # the volume mean: film_suppression forms 1 - x with x near 1 for long paths and loses 1 / s of its digits there
        s = FP.film_suppression(lams, L_BOX)
        assert np.all(np.abs(got.mean(axis=1) - s) <= 8 * 2.0 ** -53 * np.maximum(1.0, 1.0 / s) * s + 1e-15 * s)
    assert FM.film_cell_suppression(0.0, L_BOX, 0.0, 25.0) == 1.0
    # towards a wall the suppression falls: the dead layer
    prof = FM.film_cell_suppression(300.0, L_BOX, np.linspace(0, 175, 8), np.linspace(25, 200, 8))
    assert np.all(np.diff(prof) < 0) and np.allclose(prof[::-1], FM.film_cell_suppression(-300.0, L_BOX, np.linspace(0, 175, 8), np.linspace(25, 200, 8)), rtol=1e-13)


def synthetic_map():
    rng = np.random.default_rng(9)
    n = (3, 2, 2)
    rep = dict(rays=640, casts=1000, missed=0, capped=2, clamped=1, overflow=0, k_K=40, k_P=52, k_T=45, geometry_mode=1, calls=1,
               B_K=1.5, B_T=200.0, bytes=4096, seconds=1e-3)
    cells = rng.integers(0, 2 ** 40, n + (16,))
    cells[..., 0] = rng.integers(1, 60, n)
    cells[1, 1, 1] = 0
    cells[..., 14:] = 0
    fr = rng.uniform(0.2, 1.0, n)
    m = FM.normalise(cells, rep, 64, 10, 'solid', solid_fraction=fr, cell_volume=2.0, kappa_bulk=np.eye(3) * 50.0, axis=2)
    m.update(lo=np.array([0.0, -1.0, 2.0]), h=np.array([1.0, 2.0, 1.0]), n=n, cells=cells, report=rep, solid_fraction=fr,
             kappa_bulk=np.eye(3) * 50.0, kappa_global=np.eye(3), T=300.0, n_samples=64, n_list=10)
    return m


def test_file_round_trips(tmp_path):
    m = synthetic_map()
    back = FM.read_free_path_map_npz(FM.write_free_path_map_npz(FM.free_path_map_npz_path(str(tmp_path)), m))
    for key in ('kappa', 'suppression', 'N', 'p_res', 'p_wall', 'p_int', 'w_left', 'T_mean', 'cells', 'lo', 'h', 'solid_fraction',
                'kappa_bulk', 'kappa_global'):
        assert np.array_equal(back[key], m[key], equal_nan=True), key
    assert back['n'] == m['n'] and back['kind'] == 'solid' and back['axis'] == 2 and back['report'] == m['report']
    assert back['T'] == 300.0 and back['n_samples'] == 64 and back['n_list'] == 10 and back['cells'].dtype == np.int64
    v = FM.read_free_path_map_vtk(FM.write_free_path_map_vtk(FM.free_path_map_vtk_path(str(tmp_path)), m))
    assert v['n'] == m['n'] and np.array_equal(v['lo'], m['lo']) and np.array_equal(v['h'], m['h'])
    assert np.array_equal(v['N'], m['N']) and np.array_equal(v['kappa'], m['kappa'][..., 2, 2], equal_nan=True)
    assert np.array_equal(v['suppression'], m['suppression'], equal_nan=True) and np.array_equal(v['solid_fraction'], m['solid_fraction'])
    del m['solid_fraction']
    assert 'solid_fraction' not in FM.read_free_path_map_vtk(FM.write_free_path_map_vtk(str(tmp_path / 'b.vtk'), m))


def test_option_parsing():
    off = (None, 'count')
    assert FM.free_path_map_option(None) == off and FM.free_path_map_option([]) == off and FM.free_path_map_option(['0', '0', '0']) == off
    assert FM.free_path_map_option(['6', '2', '2']) == ((6, 2, 2), 'count')
    assert FM.free_path_map_option(['6', '2', '2', 'solid'], 64) == ((6, 2, 2), 'solid')
    assert FM.free_path_map_option(['256', '256', '256', 'count'], 1) == ((256, 256, 256), 'count')
    for bad in (['6'], ['6', '2'], ['6', '2', '2', 'mean'], ['6', '2', 'x'], ['6', '0', '2'], ['-1', '2', '2'], ['257', '256', '256'],
                ['6', '2', '2', 'solid', '1'], ['1.5', '2', '2']):
        with pytest.raises(ValueError, match='--free_path_map'):
            FM.free_path_map_option(bad)
    with pytest.raises(ValueError, match='requires --free_path'):
        FM.free_path_map_option(['6', '2', '2'], 0)
    from nanokappa_amd.argument_parser import initialise_parser
    base = ['--poscar_file', 'POSCAR', '--hdf_file', 'synthetic']
    args = initialise_parser().parse_args(base)
    assert FM.free_path_map_option(args.free_path_map, FP.free_path_option(args.free_path)[0]) == off          # nothing asked, nothing refused
    args = initialise_parser().parse_args(base + ['--free_path_map', '6', '2', '2', 'solid'])
    with pytest.raises(ValueError, match='requires --free_path'):
        FM.free_path_map_option(args.free_path_map, FP.free_path_option(args.free_path)[0])
    args = initialise_parser().parse_args(base + ['--free_path', '32', '--free_path_map', '6', '2', '2', 'solid'])
    assert FM.free_path_map_option(args.free_path_map, FP.free_path_option(args.free_path)[0]) == ((6, 2, 2), 'solid')


def test_weights_give_the_global_tensor():
    ct = FC.case('ttp')
    modes = FC.spread_modes(ct, 40)
    C, w = case_weights(ct, modes)
    v, tau = FC.group_vel(ct)[modes], FC.lifetimes(ct)[modes]
    D = v * tau[:, None] * 0.3
    k = FP.kappa_tensor(C, v, D, ct['tables']['QV'])
    assert np.allclose(FP._unit() * np.einsum('ma,mb->ab', w, D), k, rtol=1e-14, atol=0)


def test_restatement_tallied_and_normalised_matches_the_closed_form():
    """End to end on the CPU: the restatement's rays of 40 modes of 'ttp' (n = 64), tallied by free_map.tally and normalised
    both ways, against the closed form per slab cell: within 5 standard errors, the errors from the same per-ray terms.  In
    this box every ray ends at a reservoir or is exhausted in a single mode, so a ray that reached a reservoir arrived with
    W = 1 - T / tau (sum W g = T / tau); checked against the per-mode p_res."""
    ct = FC.case('ttp')
    modes = FC.spread_modes(ct, 40)
    ns = 64
    r = FC.run_case('ttp', modes, ns, seed=17)
    tau = FC.lifetimes(ct)[modes]
    assert set(np.unique(r['ray_end'])) <= {0, 1}
    ray_w = np.where(r['ray_end'] == 1, 1.0 - r['ray_T'] / tau[:, None], 0.0)
    assert np.abs(ray_w.sum(axis=1) - r['p_res']).max() / ns < 1e-12
    C, w = case_weights(ct, modes)
    b = np.asarray(ct['mesh']['bounds'], dtype=float)
    assert np.array_equal(b[0], np.zeros(3)) and b[1, 0] == L_BOX
    lo, h, n = FD.grid_from_bounds(b, (8, 1, 1))
    sc = FM.scales(w, FC.group_vel(ct), FC.lifetimes(ct), modes.size * ns)
    wr = np.repeat(w, ns, axis=0)
    cells = FM.tally(r['ray_x0'], r['ray_D'], r['ray_T'], ray_w, r['ray_end'], wr, lo, h, n, sc['k_K'], sc['k_P'], sc['k_T'])
    assert cells[..., 0].sum() == modes.size * ns and np.abs(cells).max() < 2 ** 62
    cf, bulk = closed_form_profile(ct, modes, w, 8)
    kb = FP.bulk_kappa(C, FC.group_vel(ct)[modes], tau, ct['tables']['QV'])
    assert abs(kb[0, 0] / (FP._unit() * bulk) - 1) < 1e-13
    full = np.ones(n)
    worst = {}
    for kind in FM.KINDS:
        m = FM.normalise(cells, sc, ns, modes.size, kind, solid_fraction=full, cell_volume=float(np.prod(h)), kappa_bulk=kb)
        val, se = profile_with_errors(r['ray_x0'], r['ray_D'], w, lo, h, n, kind, cell_fraction=full / 8.0)
        # the integers are the per-ray terms: the normalised map is the float profile to the integers' rounding
        assert np.allclose(m['kappa'][..., 0, 0], FP._unit() * val, rtol=1e-9, atol=0)
        z = np.abs(m['suppression'][:, 0, 0] - cf) / (se[:, 0, 0] / bulk)
        worst[kind] = float(z.max())
        print('%s: suppression %s, closed form %s, deviations in s.e. %s' % (kind, np.round(m['suppression'][:, 0, 0], 4), np.round(cf, 4), np.round(z, 2)))
        assert z.max() <= 5.0, (kind, z)
    # 'solid' sums back to the global tensor of the same rays
    glob = FP.kappa_tensor(C, FC.group_vel(ct)[modes], r['D'] / ns, ct['tables']['QV'])
    m = FM.normalise(cells, sc, ns, modes.size, 'solid', solid_fraction=full, cell_volume=float(np.prod(h)))
    assert np.allclose(FM.solid_mean(m['kappa'], full), glob, rtol=1e-9, atol=1e-9 * abs(glob[0, 0]))
    # the shares: everything that did not reach a reservoir was scattered intrinsically (w_left < 2^-40 per ray)
    assert np.all(m['p_wall'] == 0) and np.all(m['w_left'] < 2.0 ** -40) and np.all((m['p_res'] > 0) & (m['p_res'] < 1))
    assert np.all(m['p_res'][[0, -1], 0, 0] > m['p_res'][[3, 4], 0, 0])                  # more rays reach a wall from the cells next to it
