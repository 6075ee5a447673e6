"""Records tests/golden/free_flight_<case>.npz: the results of Engine.free_paths, free_path_map and free_path_columns on the short
lists of tests/free_path_cases.py (GOLDEN), together with the inputs of the calls (lifetimes, mode list, weights, grid).
tests/test_gpu_free_flight.py repeats the calls and compares every array byte for byte.  Only the public Engine methods are used.

    python scripts/free_path_golden.py [--out tests/golden] [--cases ttp ttrrp_k wire72]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def main():
    import free_path_cases as FC
    from test_gpu_free_path import fp_engine
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden'))
    ap.add_argument('--cases', nargs='*', default=list(FC.GOLDEN))
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    for name in a.cases:
        inp = FC.golden_inputs(name)
        eng = fp_engine(FC.golden_case(name, inp), seed=99)
        got, _ = FC.golden_calls(eng, name, inp)
        eng.close()
        path = os.path.join(a.out, 'free_flight_%s.npz' % name)
        np.savez_compressed(path, **{'in_' + k: v for k, v in inp.items()}, **got)
        end = got['n_paths_ray_end']
        print('%-8s %6d bytes  modes %s  ends %s  column ends %s  capped %d  clamped %d  overflow %d  casts %d, shared %d' % (
            name, os.path.getsize(path), inp['modes'].tolist(), np.bincount(end.ravel(), minlength=5).tolist(),
            got['n_cols_ends'].sum(axis=0).tolist(), got['n_paths_counts'][3], got['n_map_counts'][4], got['n_map_counts'][5],
            got['n_paths_counts'][1], got['n_cols_shared'][0]), flush=True)


if __name__ == '__main__':
    main()
