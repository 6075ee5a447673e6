"""Free-path sampling without a GPU: the CPU restatement of the rule (tests/free_path_cases.py) against the closed form, the
invariant, the host functions of nanokappa_amd/free_path.py, the files and the option; and the condition under which the GPU
tests may compare ray by ray."""
import numpy as np
import pytest

import free_path_cases as FC
from nanokappa_amd import free_path as FP

L_BOX = 200.0
SEED_ALL = 11


def ttp_all():
    """The restatement on 'ttp': every active mode, 64 rays, lifetimes at 300 K (shared; about 1.6e7 casts)."""
    ct = FC.case('ttp')
    return ct, FC.run_case('ttp', FC.active_modes(ct), 64, seed=SEED_ALL)


def closed_form_checks(ct, res, label):
    """The bounds of the closed-form test, for the restatement here and for the kernel in tests/test_gpu_free_path.py: every
    mode's mean D_x within 6 of its own standard errors, exactly 0 where v_x = 0, kappa_xx within 4 standard errors."""
    ml = np.asarray(res['modes'], dtype=int)
    v, tau = FC.group_vel(ct)[ml], FC.lifetimes(ct)[ml]
    D, var = FP.mean_displacement(res)
    cf = FP.film_displacement(v[:, 0], tau, L_BOX)
    z = v[:, 0] == 0
    assert z.sum() > 100 and np.all(D[z, 0] == 0.0) and np.all(cf[z] == 0.0), label + ': modes with v_x = 0 must give exactly 0'
    dev, se = np.abs(D[:, 0] - cf), np.sqrt(var[:, 0])
    worst = float(np.max(np.where(dev > 0, dev / np.maximum(se, 1e-300), 0.0)))
    print('%s: largest |mean D_x - closed form| / s.e. over %d modes: %.3f' % (label, ml.size, worst))
    assert worst <= 6.0, '%s: a mode is %.2f standard errors from the closed form' % (label, worst)
    om = np.asarray(ct['tables']['omega'], dtype=float).ravel()[ml]
    C = FP.mode_heat_capacity(om, FC.T_CASE, ct['tables']['hbar'], ct['tables']['kb'])
    k, kse = FP.kappa_tensor(C, v, D, ct['tables']['QV'], var)
    cfD = np.zeros_like(D)
    cfD[:, 0] = cf
    kcf = FP.kappa_tensor(C, v, cfD, ct['tables']['QV'])
    zk = abs(k[0, 0] - kcf[0, 0]) / kse[0, 0]
    print('%s: kappa_xx %.6f +- %.6f W/m K, closed form %.6f (%.2f s.e.)' % (label, k[0, 0], kse[0, 0], kcf[0, 0], zk))
    assert zk <= 4.0
    return k, kse, kcf


def invariant(res):
    n = float(res['n'])
    return np.abs(res['p_res'] + res['p_wall'] + res['w_left'] + res['p_int'] - n) / n


def test_restatement_matches_closed_form_on_ttp():
    ct, res = ttp_all()
    assert res['modes'].shape[0] == 4368 and res['report']['missed'] == 0 and res['report']['capped'] == 0
    k, kse, kcf = closed_form_checks(ct, res, 'restatement')
    # the rays end at the reservoirs or exhausted (v_x = 0: periodic for ever); nothing is diffuse in this box
    assert set(np.unique(res['ray_end'])) <= {0, 1} and np.all(res['p_wall'] == 0)
    assert int((res['ray_segments'].max(axis=1) > 256).sum()) == 152        # the modes the GPU test's cap of 256 cuts


def test_invariant():
    """p_res + p_wall + w_left + p_int = n per mode: every segment takes W g from the ray's weight and leaves W e = W (1 - g), so
    the sum telescopes; what is lost is the rounding of g + e = 1 (<= 2 ulp per segment, weighted by W) summed over a ray's
    segments: at most 8275 here, and the weights decay, so 1e-12 is a generous bound on the relative defect."""
    _, res = ttp_all()
    assert invariant(res).max() < 1e-12
    for name in ('ttrrp', 'ttrrp_k'):
        r = FC.parity_run(name)
        assert invariant(r).max() < 1e-12
        assert np.all(r['p_wall'] >= 0) and r['p_wall'].sum() > 0 and (r['ray_end'] == 2).any()      # diffuse ends exist there


def test_rough_cases_continue_in_another_mode():
    """'ttrrp': specular reflections carry rays into the mode of the specular map (and, with the 'k' tables, its degenerate
    partner): rays that end at a reservoir after a rough hit exist, so the continuation is exercised."""
    for name in ('ttrrp', 'ttrrp_k'):
        ct = FC.case(FC.PARITY[name]['case'])
        r = FC.parity_run(name)
        v = FC.group_vel(ct)[r['modes']]
        # a ray whose displacement is not parallel to its first mode's velocity has flown in another mode
        D = r['ray_D']
        cross = np.linalg.norm(np.cross(D, v[:, None, :]), axis=2) / (np.linalg.norm(D, axis=2) * np.linalg.norm(v, axis=1)[:, None] + 1e-300)
        assert (cross > 1e-6).sum() >= 20, name                  # (the eta = 5 angstrom walls are mostly diffuse)
    dj = FC.case('ttrrp_k')['rough']['degen_j2']
    assert (dj > -1).any()


def test_kappa_tensor_of_bulk_displacement_is_bulk_kappa():
    ct = FC.case('ttp')
    act = FC.active_modes(ct)
    v, tau = FC.group_vel(ct)[act], FC.lifetimes(ct)[act]
    C = FP.mode_heat_capacity(np.asarray(ct['tables']['omega']).ravel()[act], 300.0)
    qv = ct['tables']['QV']
    kb = FP.bulk_kappa(C, v, tau, qv)
    assert np.array_equal(FP.kappa_tensor(C, v, v * tau[:, None], qv), kb)
    assert np.allclose(kb, kb.T, rtol=1e-12, atol=0) and kb[0, 0] > 100.0          # bulk Si-like: hundreds of W/m K
    k, se = FP.kappa_tensor(C, v, v * tau[:, None], qv, np.zeros((act.size, 3)))
    assert np.array_equal(k, kb) and np.all(se == 0)
    s = FP.suppression(v * tau[:, None] * 0.5, v, tau)
    assert np.allclose(s[np.isfinite(s)], 0.5) and np.all(np.isnan(s[v == 0]))
    # heat capacity: the classical limit kb for omega -> 0, 0 for omega = 0, and the derivative of the Bose-Einstein energy
    c = FP.mode_heat_capacity(np.array([0.0, 1e-6, 50.0]), 300.0)
    K = FP.Constants()
    assert c[0] == 0.0 and abs(c[1] / K.kb - 1) < 1e-9
    n = lambda T: 1.0 / np.expm1(K.hbar * 50.0 / (K.kb * T))
    assert abs(c[2] - K.hbar * 50.0 * (n(300.5) - n(299.5))) < 1e-6 * c[2]
    # the closed form: 1 for short paths, L / (2 Lambda) for long ones, 0 displacement for v_x = 0
    assert abs(FP.film_suppression(1e-3, 200.0) - (1 - 1e-3 / 200.0)) < 1e-15
    assert abs(FP.film_suppression(2e6, 200.0) / (200.0 / 4e6) - 1) < 1e-4
    assert FP.film_displacement(0.0, 10.0, 200.0) == 0.0 and FP.film_suppression(0.0, 200.0) == 1.0


def test_summary_and_file_round_trips(tmp_path):
    ct = FC.case('ttp')
    r = FC.parity_run('ttp')
    tb = ct['tables']
    s = FP.summarise(r, tb['omega'], tb['group_vel'], FC.lifetimes(ct), tb['QV'], 300.0, axis=0, hbar=tb['hbar'], kb=tb['kb'], points=50)
    assert s['capped'] == 4500 and s['missed'] == 0 and s['invariant'] < 1e-12 and 0 < s['w_left_max'] <= 1.0
    a = s['accumulation']
    assert a['grid'].shape == (50,) and np.all(np.diff(a['bulk']) >= 0)
    assert abs(a['bulk'][-1] - s['kappa_bulk'][0, 0]) < 1e-9 * s['kappa_bulk'][0, 0]
    assert abs(a['sampled'][-1] - s['kappa'][0, 0]) < 1e-9 * abs(s['kappa'][0, 0])
    p = FP.write_k_free_path(str(tmp_path / 'k_free_path.txt'), s)
    back = FP.read_k_free_path(p)
    for key in ('kappa', 'kappa_se', 'kappa_bulk', 'grid', 'bulk', 'sampled'):
        assert np.array_equal(back[key], a[key] if key in a else s[key]), key
    assert back['T'] == 300.0 and back['N'] == r['n'] and back['missed'] == 0 and back['capped'] == 4500 and back['w_left_max'] == s['w_left_max']
    q = FP.write_free_path_npz(str(tmp_path / 'free_path.npz'), s)
    z = FP.read_free_path_npz(q)
    for key in ('modes', 'tau', 'C', 'D_mean', 'D_var', 'k_mode', 'k_mode_bulk', 'kappa', 'kappa_se', 'kappa_bulk'):
        assert np.array_equal(z[key], s[key]), key
    for key, val in s['sums'].items():
        assert np.array_equal(z['sum_' + key], val), key
    assert np.array_equal(z['suppression'], s['suppression'], equal_nan=True) and int(z['n']) == r['n']


def test_option_parsing():
    off = (0, None, FP.MAX_SEGMENTS_DEFAULT)
    assert FP.free_path_option(None) == off and FP.free_path_option([]) == off and FP.free_path_option(['0']) == off
    assert FP.free_path_option(['64']) == (64, None, 65536)
    assert FP.free_path_option(['32', '250.5']) == (32, 250.5, 65536)
    assert FP.free_path_option(['32', '300', '1000']) == (32, 300.0, 1000)
    for bad in (['-1'], ['x'], ['64', '0'], ['64', '-3'], ['64', '300', '0'], ['64', '300', '5', '6'], ['1.5'], ['64', 'nan']):
        with pytest.raises(ValueError, match='--free_path'):
            FP.free_path_option(bad)
    from nanokappa_amd.argument_parser import initialise_parser
    base = ['--poscar_file', 'POSCAR', '--hdf_file', 'synthetic']
    assert FP.free_path_option(initialise_parser().parse_args(base).free_path) == off
    assert FP.free_path_option(initialise_parser().parse_args(base + ['--free_path', '64', '300']).free_path) == (64, 300.0, 65536)


@pytest.mark.parametrize('name', sorted(FC.PARITY))
def test_gpu_comparison_inputs_do_not_hinge_on_the_rounding_of_hit_points(name):
    """The GPU tests compare ray by ray, which needs rays whose sequence of facets does not hinge on the last bit of a hit point
    (the kernel fuses x + tc v, another compiler might not): evaluated fused and unfused, the restatement must name another
    sequence of facets on fewer than 0.1 % of the rays of the inputs the GPU tests use."""
    a, b = FC.parity_run(name, fused=True), FC.parity_run(name, fused=False)
    other = float((a['ray_seq'] != b['ray_seq']).mean())
    print('%s: %d rays, %d casts, facet sequences that differ: %.4f %%' % (name, a['report']['rays'], a['report']['casts'], 100 * other))
    assert other < FC.MAX_OTHER_SEQUENCE
    assert invariant(a).max() < 1e-12
