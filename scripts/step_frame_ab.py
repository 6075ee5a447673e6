#!/usr/bin/env python3
"""Two builds of the library on the same seeds: do they compute the same?  (Written for the change that made the host side of a
step exist once -- nk_batch_enter / nk_batch_rec in nk_engine.hip; useful for any change that must leave the results alone.)

    python scripts/step_frame_ab.py --a libnanokappa_hip_parent.so --b libnanokappa_hip.so [--out profiles/step_frame_ab.txt]

Every library runs in a fresh process of its own (NK_LIBNAME is read when nanokappa_amd.engine is imported); library A runs
twice, so that what differs between two runs of ONE library is known.  Cases 'ttp' and 'ttrrp' at 30000 particles, box store and
cached store (NK_NO_BOX=1), 130 steps each as
    call      one 130-step call
    single    130 calls of one step
    resident  one 130-step call with NK_RESIDENT=1                ('ttp' only)
    group     a replica group of 3 engines (seeds 42, 43, 44)     ('ttp' only)
Across the libraries these must be EQUAL (np.array_equal): N_sv, N_emitted, N_leaving, T_sv, E_sv and the downloaded particles
matched by id; E_raw, flux_raw and the reservoir rows are summed with FP64 atomics, differ between two runs of one library, and are
held to util.RUN_TOL; the group's launch counters and timing()'s batches, halts and regrows are equal.  Should T_sv and E_sv differ
between the two runs of library A, they are held to TOL_T / TOL_E instead and the report says so.  Exit status 1 on a miss."""
import argparse
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

NSTEPS, NPART = 130, 30000
EXACT = ('N_sv', 'N_emitted', 'N_leaving')
REPRO = ('T_sv', 'E_sv')                                   # equal unless library A differs from itself
SUMMED = dict(E_raw='tol_raw', flux_raw='tol_flux', res_energy='tol_res', res_flux='tol_res')
PARTICLES = ('pid', 'mode', 'positions', 'occupation')
COUNTERS = ('batches', 'halts', 'regrows', 'box_store', 'emit_fused')
GROUP_COUNTERS = ('sweep_launches', 'tail_launches', 'member_launches')


def variants(case):
    return ('call', 'single') + (('resident', 'group') if case == 'ttp' else ())


def run_all(path):
    """Child: every setting with the library NK_LIBNAME names; everything into one .npz."""
    import util
    from nanokappa_amd.engine import EngineGroup
    out = {}

    def keep(tag, t, eng):
        for k in EXACT + REPRO + tuple(SUMMED):
            out['%s/%s' % (tag, k)] = np.asarray(t[k])
        p = eng.download()
        o = np.argsort(p['pid'], kind='stable')
        for k in PARTICLES:
            out['%s/p_%s' % (tag, k)] = np.asarray(p[k])[o]
        tm = eng.timing()
        out['%s/counters' % tag] = np.array([int(tm[k]) for k in COUNTERS], dtype=np.int64)

    for case in ('ttp', 'ttrrp'):
        ct = util.case_tables(case)
        pos, mode, occ, counter = util.random_population(ct, NPART, seed=5)
        for store in ('box', 'cached'):
            if store == 'cached':
                os.environ['NK_NO_BOX'] = '1'
            for v in variants(case):
                tag = '%s/%s/%s' % (case, store, v)
                if v == 'group':
                    engines = [util.make_engine(ct, pos, mode, occ, counter, seed=42 + r) for r in range(3)]
                    group = EngineGroup(engines)
                    ts = group.step(NSTEPS)
                    info = group.info()
                    out['%s/group' % tag] = np.array([int(info[k]) for k in GROUP_COUNTERS], dtype=np.int64)
                    for r, e in enumerate(engines):
                        keep('%s/member%d' % (tag, r), ts[r], e)
                    group.close()
                    continue
                eng = util.make_engine(ct, pos, mode, occ, counter, seed=42)
                if v == 'resident':
                    os.environ['NK_RESIDENT'] = '1'
                if v == 'single':
                    rows = [eng.step(1) for _ in range(NSTEPS)]
                    t = {k: np.concatenate([r[k] for r in rows]) for k in rows[0]}
                else:
                    t = eng.step(NSTEPS)
                os.environ.pop('NK_RESIDENT', None)
                keep(tag, t, eng)
            os.environ.pop('NK_NO_BOX', None)
    np.savez(path, **out)


def rel_row(a, b):
    """util.rel_row without the margins' bookkeeping: per step, max |a - b| / max |b|; the worst step."""
    worst = 0.0
    for s in range(a.shape[0]):
        if np.isnan(b[s]).all() and np.isnan(a[s]).all():
            continue
        if not np.array_equal(np.isnan(a[s]), np.isnan(b[s])):
            return np.inf
        worst = max(worst, float(np.nanmax(np.abs(a[s] - b[s])) / max(np.nanmax(np.abs(b[s])), 1e-300)))
    return worst


def compare(x, y, repro_exact, say):
    """x against y; returns the number of misses."""
    import util
    misses = 0
    tags = sorted(set(k.rsplit('/', 1)[0] for k in x.files if k.endswith('/N_sv')))
    for tag in tags:
        bad = []
        for k in EXACT + tuple('p_' + q for q in PARTICLES) + ('counters',):
            if not np.array_equal(x[tag + '/' + k], y[tag + '/' + k]):
                bad.append(k)
        worst = {}
        for k in REPRO:
            a, b = x[tag + '/' + k], y[tag + '/' + k]
            if repro_exact:
                if not np.array_equal(a, b):
                    bad.append(k)
            elif k == 'T_sv':
                worst[k] = float(np.max(np.abs(a - b)))
                if worst[k] > util.TOL_T:
                    bad.append(k)
            else:
                worst[k] = float(np.max(np.abs(a - b) / np.abs(b)))
                if not worst[k] < util.TOL_E:
                    bad.append(k)
        for k, tol in SUMMED.items():
            worst[k] = rel_row(x[tag + '/' + k], y[tag + '/' + k])
            if not worst[k] <= util.RUN_TOL[tol]:
                bad.append(k)
        c = x[tag + '/counters']
        say('%-34s %s  batches %d halts %d regrows %d box %d emit_fused %d | %s' % (
            tag, 'MISS ' + ','.join(bad) if bad else 'ok  ', c[0], c[1], c[2], c[3], c[4],
            '  '.join('%s %.1e' % (k, v) for k, v in worst.items())))
        misses += len(bad)
    for k in sorted(k for k in x.files if k.endswith('/group')):
        same = np.array_equal(x[k], y[k])
        say('%-34s %s  sweep_launches %d tail_launches %d member_launches %d (other library: %d %d %d)' % (
            (k, 'ok  ' if same else 'MISS') + tuple(x[k]) + tuple(y[k])))
        misses += 0 if same else 1
    return misses


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--a', default='libnanokappa_hip_parent.so', help='library A (runs twice), a file name under nanokappa_amd/')
    ap.add_argument('--b', default='libnanokappa_hip.so', help='library B')
    ap.add_argument('--out', default=None, help='append the report to this file as well')
    ap.add_argument('--child', default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        run_all(a.child)
        return 0
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    tmp = tempfile.mkdtemp()
    files = {}
    for name, lib in (('A1', a.a), ('B', a.b), ('A2', a.a)):
        files[name] = os.path.join(tmp, name + '.npz')
        env = dict(os.environ, NK_LIBNAME=lib)
        for k in ('NK_RESIDENT', 'NK_NO_BOX', 'NK_NO_ALTERNATE'):
            env.pop(k, None)
        subprocess.check_call([sys.executable, os.path.abspath(__file__), '--child', files[name]], env=env, timeout=600)
    x1, xb, x2 = (np.load(files[k]) for k in ('A1', 'B', 'A2'))
    repro_exact = all(np.array_equal(x1[k], x2[k]) for k in x1.files if k.rsplit('/', 1)[1] in REPRO)
    say('# step_frame_ab.py: A = %s, B = %s; %d particles, %d steps' % (a.a, a.b, NPART, NSTEPS))
    say('# T_sv and E_sv of two runs of A are %s: across the libraries they are held to %s' % (
        'bitwise equal' if repro_exact else 'NOT bitwise equal', 'np.array_equal' if repro_exact else 'TOL_T / TOL_E'))
    say('# --- A (first run) against A (second run): the run-to-run spread of the summed tallies')
    compare(x1, x2, repro_exact, say)
    say('# --- B against A (first run)')
    misses = compare(xb, x1, repro_exact, say)
    say('# %s' % ('all equal' if misses == 0 else '%d MISSES' % misses))
    if a.out:
        with open(a.out, 'a') as f:
            f.write('\n'.join(lines) + '\n')
    return 1 if misses else 0


if __name__ == '__main__':
    sys.exit(main())
