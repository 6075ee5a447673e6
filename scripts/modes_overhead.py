"""Cost of the mode-resolved tally (k_modes, nk_set_modes): BASELINE configs 2 and 3 at full size with the tally off and on at
every = 10 and 100, and the owner path against the forced global path at every = 10: mean step time of 100-step calls
(nk_timing.total_ms, the stream's wall time of the call).  The tally is switched on and off on the same Population,
alternating, so that every setting sees the same store placement.  The `off` figure has all its repeats listed: its spread is
what an overhead has to exceed to mean anything.

    python scripts/modes_overhead.py [--particles 1e7] [--reps 5] [--out profiles/r07_modes_overhead.txt]

--profile: instead, a short run for a kernel trace (rocprofv3 --kernel-trace --stats -- python scripts/modes_overhead.py
--profile): per config 30 steps with the tally at every = 10 and 100 frequency bands, then a few nk_tally_state calls, so that
k_modes, k_modes_accum, k_spectral and k_tally_state are timed in one run on one store.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
sys.path.insert(0, ROOT)

from spectral_overhead import build                      # the same Populations as the band pass was measured on


def profile(a):
    for cfg in a.configs:
        pop = build(cfg, int(a.particles))
        eng = pop.engine
        eng.step(20)
        pop.set_bands('frequency', 100)
        eng.set_modes(10)
        info = eng.modes_info()
        print(json.dumps(dict(config=cfg, particles=int(a.particles), modes_bytes=info['bytes'], owner_path=info['owner_path'],
                              k_E=info['k_E'])), flush=True)
        eng.step(30)
        for _ in range(3):
            eng.tally_state()
        eng.tally_modes_state()
        eng.set_modes(0)
        del pop, eng


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--particles', type=float, default=1e7)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--steps', type=int, default=100)
    ap.add_argument('--configs', nargs='*', default=['c2', 'c3'])
    ap.add_argument('--every', nargs='*', type=int, default=[10, 100])
    ap.add_argument('--profile', action='store_true')
    ap.add_argument('--out', default='')
    a = ap.parse_args()
    if a.profile:
        return profile(a)
    from nanokappa_amd.engine import MODES_GLOBAL
    lines = []
    for cfg in a.configs:
        pop = build(cfg, int(a.particles))
        eng = pop.engine
        eng.step(20)                                   # warm-up
        settings = [('off', 0, 0)] + [('every %d' % ev, ev, 0) for ev in a.every]
        settings.append(('every %d, global path forced' % a.every[0], a.every[0], MODES_GLOBAL))
        res = {s[0]: [] for s in settings}
        info = {}
        for _ in range(a.reps):
            for name, ev, flags in settings:
                eng.set_modes(ev, flags=flags)
                eng.step(10)                           # settle
                eng.step(a.steps)
                res[name].append(eng.timing()['total_ms'] / a.steps)
                info[name] = eng.modes_info()
        eng.set_modes(0)
        base = float(np.median(res['off']))
        for name, ev, flags in settings:
            med = float(np.median(res[name]))
            row = dict(config=cfg, particles=int(a.particles), modes=name, owner_path=info[name]['owner_path'] if ev else None,
                       bytes=info[name]['bytes'], step_ms_median=round(med, 5), step_ms_all=[round(x, 5) for x in res[name]],
                       overhead_pct=round(100.0 * (med / base - 1.0), 2))
            if ev:                                     # what one mode step costs: the overhead of `every` steps
                row['ms_per_mode_step'] = round((med - base) * ev, 4)
            lines.append(json.dumps(row))
            print(lines[-1], flush=True)
        del pop, eng
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
