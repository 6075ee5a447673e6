"""The field with two ranks on two GPUs (a real RCCL communicator): each field step's integer grid is all-reduced before it is
added to the accumulator, so every rank's field is the whole ensemble's -- the same bytes on the two ranks; bit for bit the
one-rank engine's integers for the freshly uploaded ensemble (identical per-particle terms); and the single-rank RUN's field up
to the rounding of the terms (the two runs' temperatures differ in their last bits).  Skipped where fewer than two GPUs are visible; the one-GPU variant with a 1-rank
communicator is test_gpu_field.py::test_field_through_single_rank_communicator."""
import multiprocessing as mp
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
NSTEPS = 20
GRID = (40, 4, 4)
CAPACITY = 1 << 21             # nk_field.capacity: above the ranks' summed slots and the one rank's, so all derive the same scales


def _grid(ct):
    from nanokappa_amd import field as FD
    return FD.grid_from_bounds(ct['mesh']['bounds'], GRID)


def _rank(rank, world, key, out_dir):
    sys.path.insert(0, HERE)
    sys.path.insert(0, os.path.join(HERE, '..'))
    from nanokappa_amd.sharding import NodeRendezvous, shard_range
    from nanokappa_amd.engine import comm_unique_id
    from util import make_engine, case_tables, random_population
    rdv = NodeRendezvous(rank, world, key, timeout=120)
    ct = case_tables('ttp')
    n = 40000
    pos, mode, occ, counter = random_population(ct, n, seed=3)
    lo, hi = shard_range(n, rank, world)
    uid = rdv.broadcast(comm_unique_id() if rank == 0 else b'')
    eng = make_engine(ct, pos[lo:hi], mode[lo:hi], occ[lo:hi], counter, seed=5, device=rank, pid_offset=lo, comm=(uid, rank, world))
    eng.set_field(*_grid(ct), 10, capacity=CAPACITY)
    st0 = eng.tally_field_state()                # the freshly uploaded particles: the same terms as in any other split of them
    info0 = eng.field_info()
    eng.step(NSTEPS)
    f = eng.field()
    st = eng.tally_field_state()
    info = eng.field_info()
    np.savez(os.path.join(out_dir, 'rank%d.npz' % rank), N=f['N'], E=f['E'], F=f['F'], samples=f['samples'], clamped=f['clamped'],
             raw=st['raw'], k=np.array([info['k_E'], info['k_F'], info['capacity']]),
             raw0=st0['raw'], clamped0=st0['clamped'], k0=np.array([info0['k_E'], info0['k_F'], info0['capacity']]))
    rdv.barrier()
    eng.close()
    rdv.close()


def test_two_ranks_field(tmp_path):
    from nanokappa_amd.engine import device_count
    if device_count() < 2:
        pytest.skip('needs two GPUs')
    ctx = mp.get_context('spawn')
    key = 'pytest_field_%d' % os.getpid()
    procs = [ctx.Process(target=_rank, args=(r, 2, key, str(tmp_path))) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(timeout=600)
        assert p.exitcode == 0
    r0, r1 = np.load(tmp_path / 'rank0.npz'), np.load(tmp_path / 'rank1.npz')
    for k in r0.files:
        assert r0[k].tobytes() == r1[k].tobytes(), k
    from util import make_engine, case_tables, random_population
    ct = case_tables('ttp')
    pos, mode, occ, counter = random_population(ct, 40000, seed=3)
    ref = make_engine(ct, pos, mode, occ, counter, seed=5)
    # Bit for bit where it can hold: the all-reduced integers of the two shards of the freshly uploaded ensemble against the
    # one-rank engine's integers of the whole of it (the same per-particle terms: every engine sees the uploaded subvolume
    # temperatures), the scales derived for one capacity on both sides (nk_field.capacity; asserted).
    ref.set_field(*_grid(ct), 10, capacity=CAPACITY)
    s0 = ref.tally_field_state()
    assert (s0['k_E'], s0['k_F']) == (int(r0['k0'][0]), int(r0['k0'][1])) and int(r0['k0'][2]) == CAPACITY == ref.field_info()['capacity']
    assert np.array_equal(r0['raw0'], s0['raw']) and int(r0['clamped0']) == s0['clamped']
    assert r0['raw0'][..., 0].sum() == 40000
    ref.set_field(*_grid(ct), 10, capacity=CAPACITY)
    ref.step(NSTEPS)
    f = ref.field()
    info = ref.field_info()
    assert int(r0['samples']) == f['samples'] == 2 and int(r0['clamped']) == f['clamped']
    assert np.array_equal(r0['N'], f['N'])
    # Against the one-rank run: the all-reduced integers are the sums of the two ranks' integers exactly, but the two RUNS are
    # not the same bits -- their subvolume temperatures come from tally sums added in different orders (and the scales follow
    # the ranks' summed capacity).  So the reals are held to the rounding of the terms on both sides plus, relative to the
    # largest cell: for E, whose terms nearly cancel, util.TOL_RUN_ERAW (two runs that sum their tallies in different orders);
    # for F the 1e-12 that test_gpu_spectral_multirank.py allows the band rows of the same two runs.
    from util import TOL_RUN_ERAW
    for key, k, tol in (('E', min(int(r0['k'][0]), info['k_E']), TOL_RUN_ERAW), ('F', min(int(r0['k'][1]), info['k_F']), 1e-12)):
        nb = f['N'] if key == 'E' else f['N'][..., None]
        assert np.all(np.abs(r0[key] - f[key]) <= 2 * nb * np.ldexp(1.0, -(k + 1)) + tol * np.max(np.abs(f[key]))), key
