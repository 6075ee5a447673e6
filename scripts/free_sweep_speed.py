"""Cost of a free-path sweep (k_free_columns, nk_free_paths_columns): device time of ONE K-column call against K single calls
(k_free_paths, nk_free_paths) with the same lifetimes in the same process, for K = 1, 4, 8, 16 `scale` columns (s log-spaced
over 0.5 .. 4; K = 1: s = 1).  BASELINE config 2's material and box (178 740 modes in the list, n = 64; planes in LDS) and the
72-sided wire of the tests (golden material, every active mode, n = 64; the face tree).  The legs alternate; five repeats after
one warm-up call each; medians and ranges (`seconds` of the calls' reports: HIP events around the launches).

    python scripts/free_sweep_speed.py [--reps 5] [--columns 1 4 8 16] [--cases c2 wire72] [--out profiles/free_sweep_notes.txt]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def engine_c2():
    from spectral_overhead import build
    from nanokappa_amd import free_path as FP
    pop = build('c2', 100000)
    return pop.engine, FP.lifetimes(pop._ph, 300.0), pop


def engine_wire72():
    import free_path_cases as FC
    from nanokappa_amd.engine import Engine
    ct = FC.case('wire72')
    eng = Engine(0, 5)
    eng.set_material(ct['tables'])
    eng.set_mesh(ct['mesh'])
    S = ct['centers'].shape[0]
    eng.set_subvolumes(ct['centers'], ct['volumes'], ct.get('kind', 0), ct['axis'], 1 if ct.get('kind', 0) == 0 else 2, np.full(S, 300.0))
    r = ct['rough']
    eng.set_rough(r['facets'], r['specularity'], r['true_spec'], r['spec_map'], r['roulette'], degen_j2=r.get('degen_j2'))
    return eng, FC.lifetimes(ct), ct


def spread(v):
    return '%.3f (%.3f .. %.3f)' % (1e3 * float(np.median(v)), 1e3 * min(v), 1e3 * max(v))


def measure(name, eng, tau, Ks, reps, n, lines):
    from nanokappa_amd import free_sweep as FS
    for K in Ks:
        scales = np.array([1.0]) if K == 1 else np.geomspace(0.5, 4.0, K)
        taus = FS.columns_scale(tau, scales)
        col = eng.free_path_columns(taus, n=n)                       # warm-up of both legs
        eng.free_paths(taus[0], n=n)
        t_col, t_one, casts_one = [], [], 0
        for _ in range(reps):
            t_col.append(eng.free_path_columns(taus, n=n)['report']['seconds'])
            ones = [eng.free_paths(t, n=n)['report'] for t in taus]
            t_one.append(sum(r['seconds'] for r in ones))
            casts_one = sum(r['casts'] for r in ones)
        rep = col['report']
        lines.append('%-7s K = %2d  geometry mode %d  %d modes  launches %d  casts shared %.4g, summed over single calls %.4g (x %.2f)'
                     % (name, K, rep['geometry_mode'], col['modes'].shape[0], rep['launches'], rep['casts_shared'], casts_one,
                        casts_one / max(rep['casts_shared'], 1)))
        lines.append('          one column call   %s ms' % spread(t_col))
        lines.append('          %2d single calls   %s ms     ratio of the medians %.2f' % (K, spread(t_one), np.median(t_one) / np.median(t_col)))
        print('\n'.join(lines[-3:]), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--columns', nargs='*', type=int, default=[1, 4, 8, 16])
    ap.add_argument('--cases', nargs='*', default=['c2', 'wire72'])
    ap.add_argument('--n', type=int, default=64)
    ap.add_argument('--out', default='')
    a = ap.parse_args()
    lines = ['device milliseconds: median (min .. max) of %d repeats, legs alternated, after one warm-up call each' % a.reps]
    for case in a.cases:
        eng, tau, keep = engine_c2() if case == 'c2' else engine_wire72()
        measure(case, eng, tau, a.columns, a.reps, a.n, lines)
        eng.close()
    if a.out:
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
