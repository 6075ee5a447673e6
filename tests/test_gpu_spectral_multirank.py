"""Band rows with two ranks on two GPUs (a real RCCL communicator): every rank's rows are the whole ensemble's -- equal on the
two ranks and to the single-rank run.  Skipped where fewer than two GPUs are visible; the one-GPU variant with a 1-rank
communicator is test_gpu_spectral.py::test_rows_through_single_rank_communicator."""
import multiprocessing as mp
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
NSTEPS = 20


def _bands(ct):
    from nanokappa_amd import spectral as SP
    b, n, _ = SP.band_map(ct['ph'].omega, 20, 'frequency')
    return b, n


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
    eng.set_bands(*_bands(ct))
    t = eng.step(NSTEPS)
    Fs, Ns = eng.tally_bands_state()
    np.savez(os.path.join(out_dir, 'rank%d.npz' % rank), F=t['band_F'], N=t['band_N'], steps=t['band_steps'], Fs=Fs, Ns=Ns)
    rdv.barrier()
    eng.close()
    rdv.close()


def test_two_ranks_band_rows(tmp_path):
    from nanokappa_amd.engine import device_count
    if device_count() < 2:
        pytest.skip('needs two GPUs')
    ctx = mp.get_context('spawn')
    key = 'pytest_bands_%d' % os.getpid()
    procs = [ctx.Process(target=_rank, args=(r, 2, key, str(tmp_path))) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(timeout=600)
        assert p.exitcode == 0
    r0, r1 = np.load(tmp_path / 'rank0.npz'), np.load(tmp_path / 'rank1.npz')
    from util import make_engine, case_tables, random_population
    ct = case_tables('ttp')
    pos, mode, occ, counter = random_population(ct, 40000, seed=3)
    ref = make_engine(ct, pos, mode, occ, counter, seed=5)
    ref.set_bands(*_bands(ct))
    t = ref.step(NSTEPS)
    Fs, Ns = ref.tally_bands_state()
    for k in ('F', 'N', 'steps', 'Fs', 'Ns'):
        assert np.array_equal(r0[k], r1[k]), k
    assert np.array_equal(r0['steps'], t['band_steps']) and np.array_equal(r0['N'], t['band_N']) and np.array_equal(r0['Ns'], Ns)
    scale = np.max(np.abs(t['band_F']))
    assert np.max(np.abs(r0['F'] - t['band_F'])) <= 1e-12 * scale
    assert np.max(np.abs(r0['Fs'] - Fs)) <= 1e-11 * np.max(np.abs(Fs))
