"""The kernels' own scalar functions (nk_device.h "lean FP64 arithmetic": nk_exp, nk_exp_small, nk_rcp, nk_occupation) and the
relaxation built from them (nk_kernels.h nk_relax), through the taps of nk_eval, against mpmath at 50 digits.  Errors are in ulps
of the reference (util.ulp_err: against the unrounded value, so that the reference's own rounding does not blur the figure).
Needs a real MI355X: `pytest -m gpu`.

Where the bounds come from.  nk_exp and nk_exp_small are pure fused-multiply-add arithmetic: a bit-exact restatement on the CPU
reached 0.884 ulp over 2e7 points of [-700, 700] (0.879 on [-40, 0]) and 0.589 ulp on [-1/8, 1/8]: the bound is 1 ulp.  nk_rcp
claims "<= 1 ulp" in nk_device.h; v_rcp_f64 has no CPU restatement, so this is its check.  The occupation's bound is derived in
test_occupation.  The relaxation is held to the project's TOL_OCC."""
import mpmath as mp
import numpy as np
import pytest

from util import golden, sub, golden_phonon, case_tables, scaled_case, rel_err, ulp_err, TOL_OCC

pytestmark = pytest.mark.gpu

LN2 = 0.6931471805599453
U = 2.0 ** -53


def exact(f, xs):
    """f (an mpmath function of an mpf) at every double of xs, 50 digits: (the double it rounds to, the remainder)."""
    xs = np.asarray(xs, dtype=float)
    hi, lo = np.zeros(xs.shape[0]), np.zeros(xs.shape[0])
    with mp.workdps(50):
        for i, x in enumerate(xs):
            v = f(mp.mpf(float(x)))
            hi[i] = float(v)
            lo[i] = float(v - mp.mpf(hi[i])) if np.isfinite(hi[i]) else 0.0
    return hi, lo


@pytest.fixture(scope='module')
def eng300():
    """Material, the 200 A box and its slices at 300 K, no reservoirs: the reference temperature T0 of the mode records' E0 is the
    middle of the live temperature range (nk_update_tau_window), 300 K.  No tap returns 1 / T0 itself; test_occupation's inputs
    at 285.5 / 285.7 and 315.8 / 316.0 K straddle the switch of nk_be only if T0 = 300."""
    from nanokappa_amd.engine import Engine
    g = sub(golden('mesh'), 'box200ttp')
    ph = golden_phonon()
    eng = Engine(0, 1)
    eng.set_material(ph.tables())
    eng.set_mesh(g)
    eng.set_subvolumes(g['subvol_center'], g['subvol_volume'], 0, int(g['slice_axis']), 1, np.full(g['subvol_center'].shape[0], 300.0))
    yield eng
    eng.close()


def test_exp(eng300):
    rng = np.random.default_rng(1)
    flips = np.array([(n + 0.5) * LN2 for n in range(-60, 61)])            # where the reduction's k = rint(x / ln 2) flips
    x = np.concatenate((rng.uniform(-700.0, 700.0, 20000), rng.uniform(-40.0, 0.0, 20000),
                        flips, np.nextafter(flips, np.inf), np.nextafter(flips, -np.inf),
                        [0.0, 2.0 ** -60, -2.0 ** -60, 0.125, -0.125]))
    got = eng300.eval('exp', x)
    hi, lo = exact(mp.exp, x)
    assert ulp_err(got, hi, lo, tag='nk_exp', bound=1.0) <= 1.0
    # far ends: nothing below the subnormals, infinity above the largest double
    # ... +0, the sign bit clear, however far below: nk_exp clamps its argument at -800 (without that the reduction loses its meaning
    # from -1e18 on and returned -0.0, +-inf and, for -inf, NaN: tests/test_free_path_edges_host.py restates it); NaN stays NaN
    far = np.array([-750.0, -1e3, -1e4, -1e17, -1e18, -1e20, -1e40, -1e45, -1e100, -1e300, -np.inf])
    low = eng300.eval('exp', far)
    assert np.array_equal(low, np.zeros(far.shape[0])) and not np.signbit(low).any(), low
    assert np.isnan(eng300.eval('exp', np.array([np.nan]))).all()
    assert np.array_equal(eng300.eval('exp', np.array([710.0])), [np.inf])
    # [-745, -700): (mostly) subnormal results, rounded once more by the ldexp: finite, non-negative, within two spacings
    xs = rng.uniform(-745.0, -700.0, 2000)
    gs = eng300.eval('exp', xs)
    assert np.all(np.isfinite(gs)) and np.all(gs >= 0.0)
    hs, ls = exact(mp.exp, xs)
    assert ulp_err(gs, hs, ls, tag='nk_exp subnormal', bound=2.0) <= 2.0


def test_exp_small(eng300):
    rng = np.random.default_rng(2)
    x = np.concatenate((rng.uniform(-0.125, 0.125, 20000),
                        [0.125, -0.125, np.nextafter(0.125, 0.0), np.nextafter(-0.125, 0.0), 0.0, 2.0 ** -60, -2.0 ** -60]))
    got = eng300.eval('exp_small', x)
    hi, lo = exact(mp.exp, x)
    assert ulp_err(got, hi, lo, tag='nk_exp_small', bound=1.0) <= 1.0


def occupation_inputs(ph):
    """(T, mode) of test_occupation: every active mode at temperatures around the switch of nk_be at T0 = 300 K (|a (1/T - 1/T0)|
    = 1/8 for the top mode at 285.6 and 315.93 K), and at 64 log-spaced temperatures."""
    active = np.nonzero(~ph.inactive_modes_mask.ravel() & (ph.omega.ravel() > 0))[0].astype(np.int32)
    Ts = np.concatenate(([200.0, 285.5, 285.7, 300.0, 315.8, 316.0, 400.0], np.geomspace(1.2, 5000.0, 64)))
    T = np.repeat(Ts, active.shape[0])
    mode = np.tile(active, Ts.shape[0])
    return T, mode


_OCC = {}


def occupation_exact(ph, T, omega):
    """1 / expm1(hbar omega / (kB T)) from the doubles, 50 digits, as (rounded double, remainder); one evaluation per distinct
    (T, omega) -- the material's symmetry leaves a few hundred distinct frequencies."""
    hi, lo = np.zeros(T.shape[0]), np.zeros(T.shape[0])
    with mp.workdps(50):
        hk = mp.mpf(float(ph.hbar)) / mp.mpf(float(ph.kb))
        for i, key in enumerate(zip(T.tolist(), omega.tolist())):
            if key not in _OCC:
                n = 1 / mp.expm1(hk * mp.mpf(key[1]) / mp.mpf(key[0]))
                h = float(n)
                _OCC[key] = (h, float(n - mp.mpf(h)))
            hi[i], lo[i] = _OCC[key]
    return hi, lo


def test_rcp(eng300):
    """nk_rcp takes no 0, inf, NaN or subnormal here: nk_rcp(inf) is NaN by construction (fma(-inf, 0, 1)), and no caller reaches
    it -- the occupation returns 0 before exp(a / T) overflows (a / T >= 700), which needs T below ~1.1 K on this material."""
    rng = np.random.default_rng(3)
    ph = golden_phonon()
    T, mode = occupation_inputs(ph)
    a = ph.hbar * ph.omega.ravel()[mode] / ph.kb
    em1 = np.expm1(a / T)
    p2 = 2.0 ** np.arange(-1000, 1001, 8)
    x = np.concatenate((rng.choice([-1.0, 1.0], 20000) * np.ldexp(rng.uniform(1.0, 2.0, 20000), rng.integers(-1000, 1001, 20000)),
                        [1.0, -1.0], p2, -p2, np.nextafter(p2, np.inf), np.nextafter(p2, 0.0), -np.nextafter(p2, np.inf),
                        np.unique(em1)))
    assert np.all(np.isfinite(x)) and np.all(np.abs(x) >= 2.0 ** -1001)
    got = eng300.eval('rcp', x)
    hi, lo = exact(lambda v: 1 / v, x)
    assert ulp_err(got, hi, lo, tag='nk_rcp', bound=1.0) <= 1.0


def test_occupation(eng300):
    """n = 1 / expm1(a / T), a = hbar omega / kB from the doubles, against nk_occupation(T, omega, E0).
    Bound: |err| / n <= (4 x + 2 x0 + 8) u E / (E - 1) + u with x = a / T, x0 = a / T0, E = exp(x), u = 2^-53 -- twice what the
    roundings of 1 / T, a * invT (and of a itself), E0, the exponential, the subtraction and the reciprocal add up to: a relative
    error eps of the exponent x is a relative error x eps of E, and a relative error of E is E / (E - 1) times that in E - 1.
    (T0 = 300 K, see eng300.)"""
    ph = golden_phonon()
    T, mode = occupation_inputs(ph)
    om = ph.omega.ravel()[mode]
    got = eng300.eval('occupation', T, mode)
    hi, lo = occupation_exact(ph, T, om)
    x, x0 = ph.hbar * om / ph.kb / T, ph.hbar * om / ph.kb / 300.0
    bound = (4 * x + 2 * x0 + 8) * U / -np.expm1(-x) + U                 # E / (E - 1) = 1 / (1 - exp(-x))
    ratio = np.abs((got - hi) - lo) / hi / bound
    assert float((ph.hbar * om / ph.kb / T).max()) < 699.0              # (none of these is cut off)
    from util import _record
    _record('rel', float(ratio.max()), 'ratio to the bound 1', depth=1, tag='nk_occupation')
    assert ratio.max() <= 1.0, 'worst ratio to the bound %g at T = %g, mode %d' % (ratio.max(), T[ratio.argmax()], mode[ratio.argmax()])
    # cut off: 0 where a / T >= 700 (exp would overflow), where T <= 0 and where omega <= 0
    top = int(np.argmax(ph.omega.ravel()))
    a_top = float(ph.hbar * ph.omega.ravel()[top] / ph.kb)
    Tc = np.array([a_top / 701.0, a_top / 1000.0, 1e-3, 0.0, -5.0])
    assert np.array_equal(eng300.eval('occupation', Tc, np.full(5, top, dtype=np.int32)), np.zeros(5))
    zero = np.nonzero(ph.omega.ravel() <= 0)[0].astype(np.int32)
    assert zero.shape[0] > 0
    assert np.array_equal(eng300.eval('occupation', np.full(zero.shape[0], 300.0), zero), np.zeros(zero.shape[0]))
    # ... and still the occupation just above the cut-off
    Tb = np.array([a_top / 698.0])
    hb, lb = exact(lambda t: 1 / mp.expm1(mp.mpf(float(ph.hbar)) / mp.mpf(float(ph.kb)) * mp.mpf(float(ph.omega.ravel()[top])) / t), Tb)
    assert rel_err(eng300.eval('occupation', Tb, np.array([top], dtype=np.int32)), hb, tag='a / T = 698', bound=4000 * U) < 4000 * U     # (4 x 698 + 13) u


def test_relax_pure_and_mixed_waves():
    """nk_relax's exp(-dt / tau) is nk_exp_small only if no lane of the wave has dt / tau >= 1/8, nk_exp otherwise: which one a
    particle gets depends on the 63 others.  dt = 1 on the test material with halved lifetimes (7.7 % of the modes over the
    threshold); the tap's waves are 64 consecutive inputs.  Waves of under-threshold modes only, of over-threshold modes only,
    and copies of the first kind with ONE lane (0, 63, 31, 17) replaced by an over-threshold particle -- so every particle is
    evaluated in a pure and in a mixed wave.  Three modes are made by hand: A with a lifetime of exactly 8 dt (dt / tau = 1/8
    belongs to the general branch), B with omega > 0 and a lifetime <= 0 (returns n0), and C with a lifetime of dt / 2: the
    halved lifetimes reach dt / tau = 0.143 only, where the short series is still good to 0.1 ulp (0.143^11 / 11! = 1e-17), so
    without C a vote that never chose the general exponential would pass."""
    from nanokappa_amd.engine import Engine
    ct0 = case_tables('ttp')
    ph = ct0['ph']
    ct = scaled_case(ct0, dt=1.0, v_scale=1.0, tau_scale=0.5)
    tb = dict(ct['tables'])
    NT = tb['lifetime'].shape[0]
    tau = tb['lifetime'].reshape(NT, -1).copy()
    omega = tb['omega'].ravel()
    rows = slice(9, 12)                                  # 290, 300, 310 K: all the temperatures of this test lie between
    assert np.array_equal(tb['T_grid'][rows], [290.0, 300.0, 310.0])
    active = ~ph.inactive_modes_mask.ravel() & (omega > 0)
    under = np.nonzero(active & (tau[rows].min(axis=0) > 8.0))[0]
    over = np.nonzero(active & (tau[rows].max(axis=0) < 8.0))[0]
    assert under.shape[0] > 3000 and over.shape[0] > 200
    mode_A, mode_B, mode_C = int(under[100]), int(under[200]), int(under[300])
    tau[:, mode_A] = 8.0
    tau[:, mode_B] = -1.0
    tau[:, mode_C] = 0.5
    under = under[(under != mode_A) & (under != mode_B) & (under != mode_C)]
    tb['lifetime'] = tau.reshape(tb['lifetime'].shape)
    S = ct['centers'].shape[0]
    T_sv = np.linspace(302.0, 298.0, S)
    eng = Engine(0, 1)
    eng.set_material(tb)
    eng.set_mesh(ct['mesh'])
    eng.set_subvolumes(ct['centers'], ct['volumes'], 0, ct['axis'], 1, T_sv)
    eng.set_params(dt=1.0, particle_density=ct['particle_density'])
    rng = np.random.default_rng(4)
    W = 64
    nP, nO = 12, 4
    b = ct['mesh']['bounds']

    def particles(modes):
        n = modes.shape[0]
        pos = b[0] + rng.random((n, 3)) * (b[1] - b[0])
        T = eng.eval('interp_T', pos)
        occ = ph.calculate_occupation(T + rng.choice([-3.0, 3.0], n), omega[modes])
        return np.column_stack((pos, occ)), modes.astype(np.int32)

    pure_a, pure_m = particles(rng.choice(under, nP * W))
    pure_m[5::W] = mode_B                                # lane 5 of every under wave: tau <= 0
    over_a, over_m = particles(rng.choice(over, nO * W))
    trig_a, trig_m = particles(np.where(np.arange(nP) % 4 == 1, mode_A, mode_C))      # the particles of modes A and C of the mixed waves
    mixed_a, mixed_m = pure_a.copy(), pure_m.copy()
    lanes = np.array([0, 63, 31, 17] * (nP // 4))
    src = np.zeros(nP, dtype=int)
    for w in range(nP):
        i = w * W + lanes[w]
        if w % 2 == 0:                                   # a particle of an all-over wave
            src[w] = rng.integers(0, nO * W)
            mixed_a[i], mixed_m[i] = over_a[src[w]], over_m[src[w]]
        else:                                            # the mode with dt / tau = 1/8 exactly, or the one with dt / tau = 2
            mixed_a[i], mixed_m[i] = trig_a[w], trig_m[w]
    a = np.concatenate((pure_a, over_a, mixed_a))
    m = np.concatenate((pure_m, over_m, mixed_m))
    got = eng.eval('relax', a, m)
    # reference: NumPy doubles on the engine's own T and tau, n0 from mpmath
    T = eng.eval('interp_T', a[:, :3])
    assert T.max() - T.min() > 3.0 and T.min() > 290.0 and T.max() < 310.0
    tl = eng.eval('lifetime', T, m)
    with mp.workdps(50):
        hk = mp.mpf(float(tb['hbar'])) / mp.mpf(float(tb['kb']))
        n0 = np.array([float(1 / mp.expm1(hk * mp.mpf(float(omega[k])) / mp.mpf(float(t)))) for k, t in zip(m, T)])
    with np.errstate(divide='ignore'):
        ref = np.where(tl > 0, n0 + (a[:, 3] - n0) * np.exp(-1.0 / tl), n0)
    nu, no = nP * W, nO * W
    is_B, is_A = m == mode_B, m == mode_A
    assert np.all(tl[is_B] <= 0) and is_B.sum() >= 2 * nP - 4
    assert np.all(tl[is_A] <= 8.0) and np.all(tl[is_A] >= 8.0 * (1 - 2 * U)) and is_A.sum() == nP // 4     # dt / tau >= 1/8: general branch
    assert np.all((tl[m == mode_C] <= 0.5) & (tl[m == mode_C] > 0.49)) and (m == mode_C).sum() == nP // 4
    assert np.all((tl[:nu] > 8.0) | is_B[:nu])                                   # the pure waves are pure
    assert np.all((tl[nu:nu + no] > 0) & (tl[nu:nu + no] < 8.0))
    for w in range(nP):                                                          # one lane over the threshold in every mixed wave
        assert ((tl[nu + no + w * W:nu + no + (w + 1) * W] <= 8.0) & (tl[nu + no + w * W:nu + no + (w + 1) * W] > 0)).sum() == 1
    assert rel_err(got[:nu], ref[:nu], tag='pure under', bound=TOL_OCC) < TOL_OCC
    assert rel_err(got[nu:nu + no], ref[nu:nu + no], tag='pure over', bound=TOL_OCC) < TOL_OCC
    assert rel_err(got[nu + no:], ref[nu + no:], tag='mixed', bound=TOL_OCC) < TOL_OCC
    assert rel_err(got[is_B], n0[is_B], tag='tau <= 0', bound=TOL_OCC) < TOL_OCC
    # the same particle in a pure and in a mixed wave: two evaluations of the exponential, both within the bound (above)
    gm = got[nu + no:]
    same = np.ones(nu, dtype=bool)
    same[np.arange(nP) * W + lanes] = False
    assert np.array_equal(a[:nu][same], mixed_a[same])
    for w in range(0, nP, 2):                             # the over particle gives the same bits in its all-over wave
        assert gm[w * W + lanes[w]] == got[nu + src[w]]
    eng.close()
