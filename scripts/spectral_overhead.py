"""Cost of the band-resolved heat-flux pass (k_spectral, nk_set_bands): BASELINE configs 2 and 3 at full size with bands off,
20 and 100 frequency bands, mean step time of 100-step calls (nk_timing.total_ms, the stream's wall time of the call).
Bands are switched on and off on the same Population, alternating, so that every setting sees the same store placement.

    python scripts/spectral_overhead.py [--particles 1e7] [--reps 3] [--out profiles/r05_spectral_overhead.txt]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
sys.path.insert(0, ROOT)


def build(cfg, total):
    import bench
    from nanokappa_amd import synthetic
    from nanokappa_amd.argument_parser import initialise_parser
    from nanokappa_amd.geometry import Geometry
    from nanokappa_amd.phonon import Phonon
    from nanokappa_amd.population import Population
    argv, species, _ = bench.config_argv(cfg, total, 200.0)
    args = initialise_parser().parse_args(argv + ['--seed', '2025', '--device', '0'])
    args.results_folder = ''
    geo = bench.quiet(Geometry, args)
    ph = Phonon(args, 0, material=synthetic.make_material(31, species, temperatures=np.arange(200.0, 401.0, 10.0)))
    return bench.quiet(Population, args, geo, ph)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--particles', type=float, default=1e7)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--steps', type=int, default=100)
    ap.add_argument('--configs', nargs='*', default=['c2', 'c3'])
    ap.add_argument('--out', default='')
    a = ap.parse_args()
    lines = []
    for cfg in a.configs:
        pop = build(cfg, int(a.particles))
        eng = pop.engine
        eng.step(20)                                   # warm-up
        res = {0: [], 20: [], 100: []}
        for _ in range(a.reps):
            for nb in (0, 20, 100):
                pop.set_bands('frequency', nb)
                eng.step(10)                           # settle (allocation of the pass's buffers)
                eng.step(a.steps)
                res[nb].append(eng.timing()['total_ms'] / a.steps)
        pop.set_bands('frequency', 0)
        base = float(np.median(res[0]))
        for nb in (0, 20, 100):
            med = float(np.median(res[nb]))
            row = dict(config=cfg, particles=int(a.particles), bands=nb, step_ms_median=round(med, 5),
                       step_ms_all=[round(x, 5) for x in res[nb]], overhead_pct=round(100.0 * (med / base - 1.0), 2))
            lines.append(json.dumps(row))
            print(lines[-1], flush=True)
        del pop, eng
    if a.out:
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
