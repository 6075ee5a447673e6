"""The three free-path calls against recorded results (tests/golden/free_flight_<case>.npz, written by
scripts/free_path_golden.py): Engine.free_paths, free_path_map and free_path_columns on short lists that reach every branch of the
flight -- the cap, periodic walls, specular turns into other modes with the degenerate partner, diffuse ends, reservoirs, the face
tree, a mode that takes no cast, a weight that runs out, a mode twice in the list, lanes with two rays, one ray and none, a workgroup with a single wave,
nine columns (a full tile and one more) -- give the recorded bytes.  The inputs of the calls (lifetimes, list, weights, grid) are
read from the fixture, so the comparison depends on the engine alone.

With the recorded start points handed back as x0 every compared number is made of additions, multiplications, divisions and fused
multiply-adds alone.  The one exception is the seeded draw of the start points, which also goes through the device's `log`: it is
compared on its own (test_seeded_draw), so a change of the math library shows there and nowhere else."""
import os

import numpy as np
import pytest

import free_path_cases as FC
from test_gpu_free_path import fp_engine

pytestmark = pytest.mark.gpu

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def recorded(name):
    def make():
        with np.load(os.path.join(GOLDEN_DIR, 'free_flight_%s.npz' % name)) as z:
            return {k: z[k] for k in z.files}
    return FC.cached(('golden', name), make)


def repeated(name):
    """golden_calls on a fresh engine with the fixture's inputs (once per process)."""
    def make():
        want = recorded(name)
        inp = {k[3:]: v for k, v in want.items() if k.startswith('in_')}
        eng = fp_engine(FC.golden_case(name, inp), seed=99)
        got = FC.golden_calls(eng, name, inp)
        eng.close()
        return got
    return FC.cached(('golden calls', name), make)


def assert_same(name, keys):
    want, got = recorded(name), repeated(name)[0]
    assert keys
    for k in keys:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        assert got[k].tobytes() == want[k].tobytes(), '%s: %s differs from the recorded bytes' % (name, k)


@pytest.mark.parametrize('name', list(FC.GOLDEN))
def test_fixture_reaches_the_branches(name):
    """What the recorded case is there for is in the recording."""
    want = recorded(name)
    p = FC.GOLDEN[name]
    modes, end = want['in_modes'], want['n_paths_ray_end']
    assert sorted(k for k in want if not k.startswith('in_')) == sorted(repeated(name)[0])
    assert modes.shape[0] == {'ttp': 6, 'ttrrp_k': 6, 'wire72': 5}[name] and modes[-1] == modes[0] and end.shape == (modes.shape[0], p['n'])
    assert (want['n_paths_ray_segments'][2] == 0).all() and (want['n_paths_ray_segments'][[0, 1, 3]] > 0).all()     # entry 2 takes no cast
    assert want['n_map_counts'][4] > 0 and want['n_map_counts'][5] == 0                         # clamped, no overflow
    assert want['n_cols_casts'].shape == (9,) and want['one_paths_ray_end'].shape == (modes.shape[0], 1)
    if name == 'ttp':
        assert (end[3] == 0).all() and want['n_paths_w_left'][3] > 0                  # weight exhausted
        assert p['n'] == 100 and want['n_paths_counts'][3] > 0 and (end == 4).any()
    if name == 'ttrrp_k':
        assert (end == 1).any() and (end == 2).any()
    if name == 'wire72':
        assert (end == 1).any() and (end == 2).any()
    if name == 'ttp':                                       # a ray whose weight runs out in one column is capped in another
        assert want['n_cols_ends'][4, 0] > 0 and want['n_cols_ends'][8, 4] > want['n_cols_ends'][4, 4]


@pytest.mark.parametrize('name', list(FC.GOLDEN))
def test_seeded_draw(name):
    """free_paths without x0 draws the recorded start points, byte for byte (this comparison also depends on the device's log)."""
    assert_same(name, ['n_x0', 'one_x0'])


@pytest.mark.parametrize('name', list(FC.GOLDEN))
@pytest.mark.parametrize('call', ['paths', 'map', 'cols'])
def test_recorded_bytes(name, call):
    """Every array of the call, with n rays per mode and with one, is the recorded one byte for byte."""
    assert_same(name, [k for k in recorded(name) if k.split('_')[1] == call])


@pytest.mark.parametrize('name', list(FC.GOLDEN))
def test_repeated_outputs(name):
    """What a call returns besides the recorded arrays repeats one of them: the start points handed in, the map's rows and rays
    (the plain call's), the rays of the column with the plain call's lifetimes."""
    got, same = repeated(name)
    assert len(same) == 2 * (1 + 13 + 5)
    for k, (a, ref) in same.items():
        assert a.dtype == got[ref].dtype and a.tobytes() == got[ref].tobytes(), '%s: %s differs from %s' % (name, k, ref)
