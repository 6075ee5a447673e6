"""Cost of a free-path map (k_free_paths<GEOM, true>, nk_free_paths_map): device time of a map call on 16^3, 64^3 and 128^3 grids against the
plain call (k_free_paths<GEOM, false>, nk_free_paths) with the same arguments in the same process.  BASELINE config 2's material and box
(178 740 modes in the list, n = 64; planes in LDS) and the 72-sided wire of the tests (golden material, every active mode, n = 64;
the face tree).  The legs alternate; five repeats after one warm-up call each; medians and ranges (`seconds` of the calls'
reports: HIP events around the launch; the map's excludes the clearing of its grid).

    python scripts/free_map_speed.py [--reps 5] [--grids 16 64 128] [--cases c2 wire72] [--out profiles/free_map_notes.txt]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from free_sweep_speed import engine_c2, engine_wire72, spread  # noqa: E402


def inputs(case, tau, keep):
    """(modes, weights [L, 3], bounds) of the default list of a case."""
    from nanokappa_amd import free_map as FM
    from nanokappa_amd import free_path as FP
    if case == 'c2':
        ph = keep._ph
        vg, om, qv, hbar, kb, b = ph.group_vel, ph.omega, ph.number_of_qpoints * ph.volume_unitcell, keep.hbar, keep.kb, keep._geo.bounds
    else:
        tb = keep['tables']
        vg, om, qv, hbar, kb, b = tb['group_vel'], tb['omega'], tb['QV'], tb['hbar'], tb['kb'], keep['mesh']['bounds']
    vg = np.asarray(vg, dtype=np.float64).reshape(-1, 3)
    modes = FP.default_modes(vg, tau)
    C = FP.mode_heat_capacity(np.asarray(om, dtype=np.float64).ravel()[modes], 300.0, hbar, kb)
    return modes, FM.weights(C, vg[modes], qv), np.asarray(b, dtype=np.float64).reshape(2, 3)


def measure(name, eng, tau, keep, grids, reps, n, lines):
    from nanokappa_amd import field as FD
    modes, w, b = inputs(name, tau, keep)
    for g in grids:
        lo, h, nc = FD.grid_from_bounds(b, (g, g, g))
        m = eng.free_path_map(tau, w, lo, h, nc, n=n, modes=modes, rays=False)       # warm-up of both legs
        eng.free_paths(tau, n=n, modes=modes)
        t_map, t_one = [], []
        for _ in range(reps):
            t_map.append(eng.free_path_map(tau, w, lo, h, nc, n=n, modes=modes, rays=False)['report']['seconds'])
            t_one.append(eng.free_paths(tau, n=n, modes=modes)['report']['seconds'])
        rep = m['report']
        filled = float((m['cells'][..., 0] > 0).mean())
        lines.append('%-7s grid %3d^3  geometry mode %d  %d modes  %d rays  %.4g casts  cells with rays %.1f %%  clamped %d  overflow %d  k_K %d'
                     % (name, g, rep['geometry_mode'], modes.shape[0], rep['rays'], rep['casts'], 100 * filled, rep['clamped'], rep['overflow'], rep['k_K']))
        lines.append('          map call     %s ms' % spread(t_map))
        lines.append('          plain call   %s ms     difference of the medians %+.3f ms, ratio %.3f'
                     % (spread(t_one), 1e3 * (np.median(t_map) - np.median(t_one)), np.median(t_map) / np.median(t_one)))
        print('\n'.join(lines[-3:]), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--grids', nargs='*', type=int, default=[16, 64, 128])
    ap.add_argument('--cases', nargs='*', default=['c2', 'wire72'])
    ap.add_argument('--n', type=int, default=64)
    ap.add_argument('--out', default='')
    a = ap.parse_args()
    lines = ['device milliseconds: median (min .. max) of %d repeats, legs alternated, after one warm-up call each' % a.reps]
    for case in a.cases:
        eng, tau, keep = engine_c2() if case == 'c2' else engine_wire72()
        measure(case, eng, tau, keep, a.grids, a.reps, a.n, lines)
        eng.close()
    if a.out:
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
