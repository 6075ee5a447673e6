"""Cost of the grouped field maps (k_field<STATE, true>, nk_set_field_groups): BASELINE config 2 at full size.

    python scripts/field_groups_overhead.py [--particles 1e7] [--reps 5] [--out profiles/r09_field_groups_overhead.txt]

Mean step time of 100-step calls (nk_timing.total_ms, the stream's wall time of the call) with the field alone and with the
groups on it, at every = 100 and 10, for a slab grid (20 x 1 x 1 cells along the slice axis, 100 frequency groups: the LDS
path) and for 64^3 cells x 8 groups (the global path).  The settings alternate on ONE Population so that every one of them
sees the same store placement; every repeat is listed.

--profile: instead, a short run for a kernel trace (rocprofv3 --kernel-trace --stats -- python scripts/field_groups_overhead.py
--profile): the slab grid with 100 frequency groups and 100 frequency bands at every = 10 for 30 steps, a few nk_tally_state
calls, then 64^3 x 8 groups for 30 steps -- the grouped and the plain k_field, k_spectral and k_tally_state timed in one run on one store.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
sys.path.insert(0, ROOT)

from spectral_overhead import build


def slab(pop):
    n = [1, 1, 1]
    n[int(pop.slice_axis)] = int(pop.n_of_subvols)
    return tuple(n)


def profile(a):
    pop = build('c2', int(a.particles))
    eng = pop.engine
    eng.step(20)
    pop.set_bands('frequency', 100)
    for n, kind, G in ((slab(pop), 'frequency', 100), ((64, 64, 64), 'frequency', 8)):
        pop.set_field(n, 10)
        pop.set_field_groups(kind, G)
        fi, gi = eng.field_info(), eng.field_groups_info()
        print(json.dumps(dict(particles=int(a.particles), grid=n, G=gi['G'], lines=gi['lines'], groups_lds_path=gi['lds_path'],
                              field_lds_path=fi['lds_path'], bytes=gi['bytes'], k_E=gi['k_E'], k_F=gi['k_F'])), flush=True)
        eng.step(30)
        for _ in range(3):
            eng.tally_state()
        g, f = eng.field_groups(), eng.field()
        print(json.dumps(dict(samples=g['samples'], ungrouped=g['ungrouped'],
                              groups_add_up_to_field=bool(np.array_equal(g['F'].sum(axis=3), f['F'])))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--particles', type=float, default=1e7)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--steps', type=int, default=100)
    ap.add_argument('--every', nargs='*', type=int, default=[100, 10])
    ap.add_argument('--profile', action='store_true')
    ap.add_argument('--out', default='')
    a = ap.parse_args()
    if a.profile:
        return profile(a)
    pop = build('c2', int(a.particles))
    eng = pop.engine
    eng.step(20)                                       # warm-up
    lines = []
    for n, G in ((slab(pop), 100), ((64, 64, 64), 8)):
        settings = [('every %d, %s' % (ev, 'field + groups' if on else 'field alone'), ev, on) for ev in a.every for on in (False, True)]
        res = {s[0]: [] for s in settings}
        info = {}
        for _ in range(a.reps):
            for name, ev, on in settings:
                pop.set_field(n, ev)
                if on:
                    pop.set_field_groups('frequency', G)
                eng.step(10)                           # settle
                eng.step(a.steps)
                res[name].append(eng.timing()['total_ms'] / a.steps)
                info[name] = eng.field_groups_info()
        for name, ev, on in settings:
            med = float(np.median(res[name]))
            row = dict(config='c2', particles=int(a.particles), grid=n, G=G, setting=name, lds_path=info[name]['lds_path'] if on else None,
                       step_ms_median=round(med, 5), step_ms_all=[round(x, 5) for x in res[name]])
            if on:
                base = float(np.median(res['every %d, field alone' % ev]))
                row['overhead_pct'] = round(100.0 * (med / base - 1.0), 2)
                row['ms_per_field_step'] = round((med - base) * ev, 4)
            lines.append(json.dumps(row))
            print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
