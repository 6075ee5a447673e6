#!/usr/bin/env python3
"""`bench.py --full` of two builds of the library, alternating, every leg of the default line (scripts/ab_libs.sh is the same idea
for one figure of one config): is B slower than A anywhere?

    python scripts/ab_full.py --a libnanokappa_hip_parent.so --b libnanokappa_hip.so --runs 5 [--out profiles/step_frame_ab.txt]

Every run is a fresh process (NK_LIBNAME selects the library), A B A B ...; then scripts/replicas_speed.py once per library.  The
legs: the headline (BASELINE config 2, 1e7 particles), `per_call` (one library call per step: where host overhead shows),
`sustained`, and `small_ensemble` on both paths (launch per step, resident kernel).  The condition is one-sided: for every leg B's
median ms per step must not exceed A's MAXIMUM over its runs -- A's own min..max is the margin.  Exit status 1 on a miss."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
LEGS = (('headline', lambda j: j['ms_per_step']),
        ('per_call', lambda j: j['per_call']['ms_per_call']),
        ('sustained', lambda j: j['sustained']['ms_per_step']),
        ('small_ensemble launch_per_step', lambda j: j['small_ensemble']['launch_per_step']['ms_per_step']),
        ('small_ensemble resident_kernel', lambda j: j['small_ensemble']['resident_kernel']['ms_per_step']))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--a', default='libnanokappa_hip_parent.so')
    ap.add_argument('--b', default='libnanokappa_hip.so')
    ap.add_argument('--runs', type=int, default=5)
    ap.add_argument('--no-replicas', action='store_true')
    ap.add_argument('--out', default=None, help='append the report to this file as well')
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    res = {a.a: [], a.b: []}
    for i in range(a.runs):
        for lib in (a.a, a.b):
            out = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--full', '--no-cpu-baseline'], cwd=ROOT,
                                 env=dict(os.environ, NK_LIBNAME=lib), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=420)
            if out.returncode != 0:
                sys.stderr.write(out.stderr.decode()[-2000:])
                raise SystemExit('bench.py failed with %s (status %d)' % (lib, out.returncode))
            j = json.loads(out.stdout.decode().strip().split('\n')[-1])
            res[lib].append(j)
            # (beside the legs: the sweep's own time and the speed of the memory the store was placed in -- profiles/r03_notes.txt (9), (17))
            say('run %d %-28s %s  | k_sweep %.5f ms, store placed at %.0f GB/s of %d allocations timed' % (
                i, lib, '  '.join('%s %.5f' % (n.split()[-1], f(j)) for n, f in LEGS), j['roofline']['kernel_ms'],
                j['store_placement']['kept_copy_GBps'], j['store_placement']['allocations_timed']))
    say('# ab_full.py: bench.py --gpus 1 --full --no-cpu-baseline, %d runs each, alternating; A = %s, B = %s; ms per step (per call)' % (a.runs, a.a, a.b))
    misses = 0
    for name, f in LEGS:
        va, vb = np.array([f(j) for j in res[a.a]]), np.array([f(j) for j in res[a.b]])
        ok = np.median(vb) <= va.max()
        misses += 0 if ok else 1
        say('%-32s A median %.5f [%.5f .. %.5f]  B median %.5f [%.5f .. %.5f]  %s   A %s  B %s' % (
            name, np.median(va), va.min(), va.max(), np.median(vb), vb.min(), vb.max(), 'ok' if ok else 'MISS: B median above A max',
            ' '.join('%.5f' % v for v in va), ' '.join('%.5f' % v for v in vb)))
    for tag, lib in (('A', a.a), ('B', a.b)):
        say('headline %s: %.4e phonon-steps/s (median of the runs\' values; each the median of %d regions)' % (
            tag, float(np.median([j['value'] for j in res[lib]])), res[lib][0]['repeats']))
    if not a.no_replicas:
        for tag, lib in (('A', a.a), ('B', a.b)):
            out = subprocess.run([sys.executable, os.path.join(ROOT, 'scripts', 'replicas_speed.py')], cwd=ROOT, env=dict(os.environ, NK_LIBNAME=lib),
                                 stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=420)
            if out.returncode != 0:
                sys.stderr.write(out.stderr.decode()[-2000:])
                raise SystemExit('replicas_speed.py failed with %s (status %d)' % (lib, out.returncode))
            say('# replicas_speed.py, %s = %s' % (tag, lib))
            for l in out.stdout.decode().strip().split('\n'):
                say(l)
    say('# %s' % ('no leg slower' if misses == 0 else '%d legs MISS' % misses))
    if a.out:
        with open(a.out, 'a') as f:
            f.write('\n'.join(lines) + '\n')
    return 1 if misses else 0


if __name__ == '__main__':
    sys.exit(main())
