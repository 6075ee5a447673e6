#!/usr/bin/env python3
"""Replica groups against the same engines stepped one after another (bench.py stays as it is; this is the group's own measurement).

BASELINE config 1 at its own size (1e5 particles, 31^3 x 6 modes, box 200 A, slice 20, T T P), R in {1, 2, 4, 8, 16} engines under
seeds 2025 .. 2025 + R - 1 in ONE process.  Two legs over the SAME engines (both keep the members at the same step):
    sequential   for e in engines: e.step(n)        -- nk_step, the machine code of the launch-per-step path
    group        EngineGroup(engines).step(n)       -- one k_sweep_group + one k_tail_group per step for all of them
alternated, --repeats timed regions of --steps steps each per leg, after an untimed ramp of --ramp steps (as bench.py: the device
leaves the host-side set-up in a low power state).  Aggregate phonon-steps/s = particles of all members summed over the region's
steps / wall time of the region (stream drained at both ends: every library call ends with a wait).

    python scripts/replicas_speed.py --out profiles/r08_replicas_speed.txt
    rocprofv3 --kernel-trace --stats -d DIR -- python scripts/replicas_speed.py --only-group 8 --steps 300     (kernel statistics)
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
sys.path.insert(0, ROOT)


_SHARED = {}          # geometry and material, built once for all R


def build_engines(R, particles, mesh_n, seed0):
    import bench
    from nanokappa_amd import synthetic
    from nanokappa_amd.argument_parser import initialise_parser
    from nanokappa_amd.geometry import Geometry
    from nanokappa_amd.phonon import Phonon
    from nanokappa_amd.population import Population
    argv, species, desc = bench.config_argv('c2', particles, 200.0)
    pops = []
    for k in range(R):
        args = initialise_parser().parse_args(argv + ['--seed', str(seed0 + k), '--device', '0'])
        args.results_folder = ''
        if 'geo' not in _SHARED:
            _SHARED['geo'] = bench.quiet(Geometry, args)
            _SHARED['ph'] = Phonon(args, 0, material=synthetic.make_material(mesh_n, species, temperatures=np.arange(200.0, 401.0, 10.0)))
        pops.append(bench.quiet(Population, args, _SHARED['geo'], _SHARED['ph'], None, None))
    return pops, desc


def region(fn, n):
    t0 = time.perf_counter()
    ts = fn(n)
    dt = time.perf_counter() - t0
    return dt, float(sum(t['N_sv'].sum() for t in ts))


def measure(R, a, out):
    from nanokappa_amd.engine import EngineGroup
    pops, desc = build_engines(R, a.particles, a.mesh_n, 2025)
    engines = [p.engine for p in pops]
    group = EngineGroup(engines)
    legs = {'sequential': lambda n: [e.step(n) for e in engines], 'group': lambda n: group.step(n)}
    for _ in range(max(a.ramp, 0) // 100):
        group.step(100)
    for name in ('sequential', 'group'):               # one untimed region of each leg
        legs[name](a.steps)
    res = {'sequential': [], 'group': []}
    for _ in range(a.repeats):
        for name in ('sequential', 'group'):
            dt, ps = region(legs[name], a.steps)
            res[name].append((ps / dt, 1e3 * dt / a.steps))
    info = group.info()
    tm = engines[0].timing()
    line = {}
    for name in ('sequential', 'group'):
        v = np.array([r[0] for r in res[name]])
        ms = np.array([r[1] for r in res[name]])
        line[name] = dict(median=float(np.median(v)), lo=float(v.min()), hi=float(v.max()), ms=float(np.median(ms)))
    ratio = line['group']['median'] / line['sequential']['median']
    spread = (line['sequential']['hi'] - line['sequential']['lo']) / line['sequential']['median']
    out.write('R %2d  sequential %.3e (min %.3e max %.3e) phonon-steps/s, %.4f ms per step of all members | group %.3e (min %.3e max %.3e), %.4f ms '
              '| group / sequential %.3f (spread of the sequential leg %.1f %%) | k_sweep_group %.4f ms (%d workgroups)  k_tail_group %.4f ms (%d) '
              '| solo k_sweep %.4f ms, tail %.4f ms | halted %d, member launches %d\n'
              % (R, line['sequential']['median'], line['sequential']['lo'], line['sequential']['hi'], line['sequential']['ms'],
                 line['group']['median'], line['group']['lo'], line['group']['hi'], line['group']['ms'], ratio, 100.0 * spread,
                 info['sweep_kernel_ms'], info['grid_sweep'], info['tail_kernel_ms'], info['grid_tail'],
                 tm['step_kernel_ms'], tm['events_kernel_ms'], info['halted'], info['member_launches']))
    out.flush()
    group.close()
    for e in engines:
        e.close()
    return line, ratio, spread


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--R', type=int, nargs='*', default=[1, 2, 4, 8, 16])
    ap.add_argument('--steps', type=int, default=500)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--ramp', type=int, default=400)
    ap.add_argument('--particles', type=int, default=100000)
    ap.add_argument('--mesh_n', type=int, default=31)
    ap.add_argument('--out', default=None, help='append the result lines to this file as well')
    ap.add_argument('--only-group', type=int, default=0, metavar='R', help='no timing: R engines, --steps grouped steps (for a profiler)')
    a = ap.parse_args()
    if a.only_group > 0:
        from nanokappa_amd.engine import EngineGroup
        pops, _ = build_engines(a.only_group, a.particles, a.mesh_n, 2025)
        g = EngineGroup([p.engine for p in pops])
        done = 0
        while done < a.steps:
            n = min(100, a.steps - done)
            g.step(n)
            done += n
        print(g.info())
        g.close()
        return

    class Tee(object):
        def __init__(self, f):
            self.f = f

        def write(self, s):
            sys.stdout.write(s)
            if self.f:
                self.f.write(s)

        def flush(self):
            sys.stdout.flush()
            if self.f:
                self.f.flush()

    f = open(a.out, 'w') if a.out else None
    out = Tee(f)
    out.write('# replica groups against the same engines stepped one after another: BASELINE config 1, %d particles per member, %d^3 x 6 modes\n'
              % (a.particles, a.mesh_n))
    out.write('# %d timed regions of %d steps per leg, legs alternated, after %d untimed steps; aggregate phonon-steps/s (median, min, max)\n'
              % (a.repeats, a.steps, max(a.ramp, 0) // 100 * 100))
    results = {}
    for R in a.R:
        results[R] = measure(R, a, out)
    if 8 in results:
        line, ratio, spread = results[8]
        out.write('# R = 8: group / sequential = %.3f; the requirement (more than the spread of the sequential leg, %.1f %%): %s; aggregate %.3e against '
                  'the aim of 1.5e10: %s\n' % (ratio, 100.0 * spread, 'met' if ratio - 1.0 > spread else 'NOT met', line['group']['median'],
                                               'met' if line['group']['median'] >= 1.5e10 else 'not met'))
    if 1 in results:
        out.write('# R = 1: group / nk_step = %.3f (the members\' NkDev read from constant memory instead of the kernel arguments)\n' % results[1][1])
    if f:
        f.close()


if __name__ == '__main__':
    main()
