"""Speed of the kinetic flights (k_kinetic, nk_kinetic_flights) against the free-path call (k_free_paths, nk_free_paths) on the same
geometry in the same process: casts per second of device time.  BASELINE config 2's material and box (planes in LDS) and the
72-sided wire of the tests (golden material; the face tree), with the lifetimes at 300 K and with a sixteenth of them.  The legs
alternate; five repeats after one warm-up call each; medians and ranges (`seconds` of the calls' reports: HIP events around the
launch).  On config 2 it also prints kappa_eff with its standard error and the per-slice temperature profile.

    python scripts/kinetic_speed.py [--reps 5] [--n 1048576] [--cases c2 wire72] [--run-steps 6000] [--out profiles/kinetic_notes.txt]

Run it once more with NK_LIBNAME=libnanokappa_hip_nested.so (make -C nanokappa_amd/csrc kinetic-nested) for the nested per-ray loop
the flat lane loop is measured against."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from free_sweep_speed import engine_c2, engine_wire72, spread  # noqa: E402


def rate(reports):
    r = [x['casts'] / x['seconds'] for x in reports]
    return '%.3g (%.3g .. %.3g) casts/s' % (np.median(r), min(r), max(r))


def measure(name, eng, tau, c, n, n_fp, reps, lines):
    for label, scale in (('tau', 1.0), ('tau/16', 1.0 / 16.0)):
        t = np.where(tau > 0, tau * scale, tau)
        eng.kinetic_flights(t, c, n=n)                                # warm-up of both legs
        eng.free_paths(t, n=n_fp)
        kin, fp = [], []
        for _ in range(reps):
            kin.append(eng.kinetic_flights(t, c, n=n)['report'])
            fp.append(eng.free_paths(t, n=n_fp)['report'])
        k = kin[0]
        lines.append('%-7s %-7s geometry mode %d  kinetic: %d rays, %.4g events, %.4g casts, %.1f casts per ray, grid %d, lds bins %d; lost %d missed %d capped %d'
                     % (name, label, k['geometry_mode'], k['rays'], k['events'], k['casts'], k['casts'] / k['rays'], k['grid'], k['lds_bins'],
                        k['lost'], k['missed'], k['capped']))
        lines.append('          kinetic flights  %s ms   %s' % (spread([x['seconds'] for x in kin]), rate(kin)))
        lines.append('          free paths       %s ms   %s   (%d rays, %.4g casts)' % (spread([x['seconds'] for x in fp]), rate(fp), fp[0]['rays'], fp[0]['casts']))
        print('\n'.join(lines[-3:]), flush=True)


def config2(pop, n, lines):
    s = pop.kinetic_flights(n=n, write=False)
    lines.append('config 2: T = %.1f K, N = %d per source: kappa_eff = %.4f +- %.4f W/m K (bulk %.2f, free-path closed form %.4f); device time %.4f s; lost %d missed %d capped %d'
                 % (s['T'], s['n'], s['kappa_eff'], s['kappa_eff_se'], s['kappa_bulk'], s['kappa_free_path'], s['report']['seconds'],
                    s['lost'].sum(), s['missed'].sum(), s['capped'].sum()))
    lines.append('          G (W/K) ' + np.array2string(s['G'], precision=6) + '  +- ' + np.array2string(s['G_se'], precision=3))
    lines.append('          T_ref + dT per slice (K): ' + ' '.join('%.4f' % x for x in s['T_ref'] + s['dT']))
    lines.append('          q_x per slice (W/m^2):    ' + ' '.join('%.5g' % x for x in s['q'][:, 0]))
    lines.append('          kappa from the mean q_x and the reservoirs\' difference: %.4f W/m K'
                 % (abs(s['q'][:, 0].mean()) * s['L'] * 1e-10 / abs(s['T_f'][0] - s['T_f'][1])))
    print('\n'.join(lines[-5:]), flush=True)
    return s


def against_run(kin, steps, samples, lines):
    """The per-slice temperatures of the kinetic flights beside those of a run of config 2 at full size: `steps` steps, then the
    mean of `samples` readings of the subvolume temperatures 100 steps apart."""
    import bench
    from spectral_overhead import build
    pop = build('c2', 1e7)
    bench.quiet(pop.run, steps, pop._geo, pop._ph)
    T = []
    for _ in range(samples):
        bench.quiet(pop.run, 100, pop._geo, pop._ph)
        T.append(np.array(pop.subvol_temperature, dtype=np.float64))
    T = np.array(T)
    m, se = T.mean(axis=0), T.std(axis=0, ddof=1) / np.sqrt(samples)
    k = kin['T_ref'] + kin['dT']
    lines.append('config 2, the run (1e7 particles, %d steps, then %d readings 100 steps apart), T per slice (K): ' % (steps, samples) + ' '.join('%.4f' % x for x in m))
    lines.append('          standard error of those means at most %.4f K (readings 100 steps apart are correlated: a lower bound)' % se.max())
    lines.append('          kinetic flights minus run (K): ' + ' '.join('%+.4f' % x for x in k - m))
    lines.append('          slope per slice: kinetic %.5f K, run %.5f K; jump at the hot contact: kinetic %.4f K, run %.4f K'
                 % (np.polyfit(np.arange(k.size), k, 1)[0], np.polyfit(np.arange(m.size), m, 1)[0], kin['T_f'][0] - (k[0] - 0.5 * (k[1] - k[0])),
                    kin['T_f'][0] - (m[0] - 0.5 * (m[1] - m[0]))))
    print('\n'.join(lines[-4:]), flush=True)
    pop.engine.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--n', type=int, default=1 << 20)
    ap.add_argument('--cases', nargs='*', default=['c2', 'wire72'])
    ap.add_argument('--run-steps', type=int, default=0, help='also run config 2 at full size for so many steps and lay its subvolume temperatures beside the profile')
    ap.add_argument('--out', default='')
    a = ap.parse_args()
    from nanokappa_amd import kinetic as KN
    lines = ['library %s; device milliseconds: median (min .. max) of %d repeats, legs alternated, after one warm-up call each'
             % (os.environ.get('NK_LIBNAME', 'libnanokappa_hip.so'), a.reps)]
    for case in a.cases:
        eng, tau, keep = engine_c2() if case == 'c2' else engine_wire72()
        if case == 'c2':
            ph = keep._ph
            c = KN.heat_capacity(ph.omega, 300.0, ph.number_of_qpoints * ph.volume_unitcell, keep.hbar, keep.kb)
            measure(case, eng, tau, c, a.n, 64, a.reps, lines)
            kin = config2(keep, 4 * a.n, lines)
            if a.run_steps > 0:
                eng.close()
                against_run(kin, a.run_steps, 40, lines)
        else:
            import kinetic_cases as K
            measure(case, eng, tau, K.heat_capacity(keep), a.n, 4096, a.reps, lines)
        eng.close()
    if a.out:
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
