"""Cost of the spatial field pass (k_field, nk_set_field): BASELINE configs 2 and 3 at full size with the field off and on,
for grids of 16^3, 64^3 and 128^3 cells at every = 10 and 100, and the LDS path against the forced global path at 16^3: mean
step time of 100-step calls (nk_timing.total_ms, the stream's wall time of the call).  The field is switched on and off on
the same Population, alternating, so that every setting sees the same store placement.  The `off` figure has all its repeats
listed: its spread is what an overhead has to exceed to mean anything.

    python scripts/field_overhead.py [--particles 1e7] [--reps 5] [--out profiles/r06_field_overhead.txt]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
sys.path.insert(0, ROOT)

from spectral_overhead import build                      # the same Populations as the band pass was measured on


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--particles', type=float, default=1e7)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--steps', type=int, default=100)
    ap.add_argument('--configs', nargs='*', default=['c2', 'c3'])
    ap.add_argument('--grids', nargs='*', type=int, default=[16, 64, 128])
    ap.add_argument('--every', nargs='*', type=int, default=[10, 100])
    ap.add_argument('--out', default='')
    a = ap.parse_args()
    from nanokappa_amd.engine import FIELD_GLOBAL
    from nanokappa_amd import field as FD
    lines = []
    for cfg in a.configs:
        pop = build(cfg, int(a.particles))
        eng = pop.engine
        eng.step(20)                                   # warm-up
        settings = [('off', 0, 0, 0)]
        for g in a.grids:
            for ev in a.every:
                settings.append(('%d^3 every %d' % (g, ev), g, ev, 0))
        settings.append(('%d^3 every %d, global path forced' % (a.grids[0], a.every[0]), a.grids[0], a.every[0], FIELD_GLOBAL))
        res = {s[0]: [] for s in settings}
        path = {}
        for _ in range(a.reps):
            for name, g, ev, flags in settings:
                if g:
                    lo, h, n = FD.grid_from_bounds(pop._geo.bounds, (g, g, g))
                    eng.set_field(lo, h, n, ev, flags=flags)
                else:
                    eng.set_field((0, 0, 0), (1, 1, 1), (0, 0, 0), 1)
                eng.step(10)                           # settle
                eng.step(a.steps)
                res[name].append(eng.timing()['total_ms'] / a.steps)
                path[name] = eng.field_info()['lds_path'] if g else None
        eng.set_field((0, 0, 0), (1, 1, 1), (0, 0, 0), 1)
        base = float(np.median(res['off']))
        for name, g, ev, flags in settings:
            med = float(np.median(res[name]))
            row = dict(config=cfg, particles=int(a.particles), field=name, lds_path=path[name], step_ms_median=round(med, 5),
                       step_ms_all=[round(x, 5) for x in res[name]], overhead_pct=round(100.0 * (med / base - 1.0), 2))
            if g:                                      # what one field step costs: the overhead of `every` steps
                row['ms_per_field_step'] = round((med - base) * ev, 4)
            lines.append(json.dumps(row))
            print(lines[-1], flush=True)
        del pop, eng
    if a.out:
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
