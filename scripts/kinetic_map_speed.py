"""Speed of the kinetic maps (k_kinetic<.., false, true>, nk_kinetic_flights_map) beside the plain call (k_kinetic<.., false, false>,
nk_kinetic_flights) on the same geometry in the same process, by the protocol of scripts/kinetic_speed.py: BASELINE config 2's
material and box and the 72-sided wire, the lifetimes at 300 K and a sixteenth of them, N = 2^20 rays per source, legs alternated,
five repeats after one warm-up call each, medians and ranges of the reports' `seconds` (HIP events around the launch).  The legs:
the plain call; with --other-lib, the plain call of another build of the library (the parent commit's, to see that the plain
instantiations still run at their speed); the map at 16^3 cells; the map at 64^3 cells (both over the mesh's bounds).  On config 2
it also prints T(x) of a 20 x 1 x 1 map from 8 batches beside the per-slice profile of the same flights.

    python scripts/kinetic_map_speed.py [--reps 5] [--n 1048576] [--cases c2 wire72] [--other-lib PATH] [--result-n 4194304]
                                        [--out profiles/kinetic_map_notes.txt]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from free_sweep_speed import engine_c2, engine_wire72, spread  # noqa: E402
from kinetic_groups_speed import other_engine  # noqa: E402

GRIDS = ((16, 16, 16), (64, 64, 64))


def measure(name, eng, other, bounds, tau, c, n, reps, lines):
    from nanokappa_amd import field as FD
    for label, scale in (('tau', 1.0), ('tau/16', 1.0 / 16.0)):
        t = np.where(tau > 0, tau * scale, tau)
        legs = [('plain', eng, None)]
        if other is not None:
            legs.append(('plain, other library', other, None))
        legs += [('map %d^3' % nc[0], eng, FD.grid_from_bounds(bounds, nc)) for nc in GRIDS]
        call = lambda e, g: e.kinetic_flights(t, c, n=n) if g is None else e.kinetic_flights(t, c, n=n, grid=g)
        res = {k: [] for k, _, _ in legs}
        last = {}
        for k, e, g in legs:                                          # warm-up of every leg
            call(e, g)
        for _ in range(reps):
            for k, e, g in legs:
                last[k] = call(e, g)
                res[k].append(last[k]['report'])
        p = res['plain'][0]
        lines.append('%-7s %-7s geometry mode %d  %d rays, %.4g events, grid %d, lds bins %d' % (name, label, p['geometry_mode'], p['rays'], p['events'], p['grid'], p['lds_bins']))
        base = float(np.median([x['seconds'] for x in res['plain']]))
        for k, _, g in legs:
            r = res[k]
            rows = np.delete(last[k]['rows'], 25, axis=1)
            same = np.array_equal(last[k]['sub'], last['plain']['sub']) and np.array_equal(rows, np.delete(last['plain']['rows'], 25, axis=1))
            more = ''
            if g is not None:
                m = last[k]['map']
                more = '; cells sum to sub: %s; %d of %d lines hold a word; clamped %d' % (
                    np.array_equal(m.reshape(m.shape[0], -1, 4).sum(axis=1), last[k]['sub'].sum(axis=1)), int((m != 0).any(axis=-1).sum()),
                    m.shape[0] * m.shape[1] * m.shape[2] * m.shape[3], int(last[k]['clamped'].sum()))
            med = float(np.median([x['seconds'] for x in r]))
            lines.append('          %-22s %s ms   %+6.1f %% on the plain call; sub and rows equal to the plain call\'s: %s%s'
                         % (k, spread([x['seconds'] for x in r]), 100.0 * (med / base - 1.0), same, more))
        if other is not None:
            o = [x['seconds'] for x in res['plain, other library']]
            lines.append('          the plain call\'s median lies inside the other library\'s five repeats or below its fastest: %s' % (base <= max(o)))
        print('\n'.join(lines[-len(legs) - 2:]), flush=True)


def config2(pop, n, lines):
    """T(x) of a 20 x 1 x 1 map of config 2 beside the per-slice profile of the same pooled flights."""
    S = len(pop.subvol_temperature)
    m = pop.kinetic_map((S, 1, 1), n=n, batches=8, write=False)
    s = m['summary']
    lines.append('config 2: T = %.1f K, N = %d per source in %d batches, map of %d x 1 x 1 cells over the bounds: kappa_eff = %.4f +- %.4f W/m K; clamped %d'
                 % (s['T'], s['n'], m['batches'], S, s['kappa_eff'], s['kappa_eff_se'], int(m['clamped'].sum())))
    lines.append('          T per cell (K):          ' + ' '.join('%.4f' % x for x in m['T'][:, 0, 0]))
    lines.append('          its standard error (K):  ' + ' '.join('%.4f' % x for x in m['T_se'][:, 0, 0]))
    lines.append('          T_ref + dT per slice (K): ' + ' '.join('%.4f' % x for x in s['T_ref'] + s['dT']))
    lines.append('          q_x per cell (W/m^2):    ' + ' '.join('%.5g' % x for x in m['q'][:, 0, 0, 0]))
    lines.append('          the cells\' dwell words equal the slices\' bit for bit: %s; largest |T cell - T slice| %.2e K'
                 % (np.array_equal(m['map'][:, :, 0, 0, 0] * 2.0 ** -s['report']['k_t'], s['dwell']),
                    float(np.max(np.abs(m['T'][:, 0, 0] - (s['T_ref'] + s['dT']))))))
    print('\n'.join(lines[-6:]), flush=True)
    return m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--n', type=int, default=1 << 20)
    ap.add_argument('--cases', nargs='*', default=['c2', 'wire72'])
    ap.add_argument('--other-lib', default='')
    ap.add_argument('--result-n', type=int, default=0, help='also print config 2\'s T(x) of a 20 x 1 x 1 map at so many rays per source')
    ap.add_argument('--out', default='')
    a = ap.parse_args()
    from nanokappa_amd import kinetic as KN
    lines = ['device milliseconds: median (min .. max) of %d repeats, legs alternated, after one warm-up call each; N = %d rays per source' % (a.reps, a.n)]
    if a.other_lib:
        lines.append('other library: %s' % os.path.basename(a.other_lib))
    for case in a.cases:
        make = engine_c2 if case == 'c2' else engine_wire72
        eng, tau, keep = make()
        other = None
        if a.other_lib:
            other, _ = other_engine(case, os.path.abspath(a.other_lib))
        if case == 'c2':
            ph = keep._ph
            c = KN.heat_capacity(ph.omega, 300.0, ph.number_of_qpoints * ph.volume_unitcell, keep.hbar, keep.kb)
            measure(case, eng, other, keep._geo.bounds, tau, c, a.n, a.reps, lines)
            if a.result_n > 0:
                config2(keep, a.result_n, lines)
        else:
            import kinetic_cases as K
            measure(case, eng, other, np.asarray(keep['mesh']['bounds'], dtype=np.float64).reshape(2, 3), tau, K.heat_capacity(keep), a.n, a.reps, lines)
        eng.close()
        if other is not None:
            other.close()
        if a.out:                                                     # (after every case: a run cut short keeps what it measured)
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, 'w') as f:
                f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
