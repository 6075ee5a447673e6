"""The mode-resolved tally with two ranks on two GPUs (a real RCCL communicator): only the sample's header is summed over the
ranks per mode step (every rank takes or drops the same samples); the accumulators stay per rank and are summed once, at
read-out, so every rank reads the whole ensemble's table -- the same bytes on the two ranks; state mode sums the integers
over the ranks: bit for bit the one-rank engine's integers for the freshly uploaded ensemble.  Skipped where fewer than two GPUs
are visible; the one-GPU variant with a 1-rank communicator is test_gpu_modes.py::test_modes_through_single_rank_communicator."""
import multiprocessing as mp
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
NSTEPS = 20
CAPACITY = 1 << 21             # nk_modes.capacity: above the ranks' summed slots and the one rank's, so all derive the same scale


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
    eng.set_modes(10, capacity=CAPACITY)
    st0 = eng.tally_modes_state()                # the freshly uploaded particles: the same terms as in any other split of them
    info0 = eng.modes_info()
    eng.step(NSTEPS)
    m = eng.modes()
    st = eng.tally_modes_state()
    info = eng.modes_info()
    np.savez(os.path.join(out_dir, 'rank%d.npz' % rank), N=m['N'], E=m['E'], samples=m['samples'], skipped=m['skipped'],
             N_raw=st['N_raw'], E_raw=st['E_raw'], k=np.array([info['k_E'], info['capacity']]),
             N_raw0=st0['N_raw'], E_raw0=st0['E_raw'], k0=np.array([info0['k_E'], info0['capacity']]))
    rdv.barrier()
    eng.close()
    rdv.close()


def test_two_ranks_modes(tmp_path):
    from nanokappa_amd.engine import device_count
    if device_count() < 2:
        pytest.skip('needs two GPUs')
    ctx = mp.get_context('spawn')
    key = 'pytest_modes_%d' % os.getpid()
    procs = [ctx.Process(target=_rank, args=(r, 2, key, str(tmp_path))) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(timeout=600)
        assert p.exitcode == 0
    r0, r1 = np.load(tmp_path / 'rank0.npz'), np.load(tmp_path / 'rank1.npz')
    for k in r0.files:
        assert r0[k].tobytes() == r1[k].tobytes(), k
    from util import make_engine, case_tables, random_population, TOL_RUN_ERAW
    ct = case_tables('ttp')
    pos, mode, occ, counter = random_population(ct, 40000, seed=3)
    ref = make_engine(ct, pos, mode, occ, counter, seed=5)
    ref.set_modes(10, capacity=CAPACITY)
    s0 = ref.tally_modes_state()
    assert s0['k_E'] == int(r0['k0'][0]) and int(r0['k0'][1]) == CAPACITY == ref.modes_info()['capacity']
    assert np.array_equal(r0['N_raw0'], s0['N_raw']) and np.array_equal(r0['E_raw0'], s0['E_raw'])
    assert r0['N_raw0'].sum() == 40000
    ref.step(NSTEPS)
    m = ref.modes()
    assert int(r0['samples']) == m['samples'] == 2 and int(r0['skipped']) == m['skipped'] == 0
    assert np.array_equal(r0['N'], m['N'])
    # the two RUNS are not the same bits (their subvolume temperatures come from tally sums added in different orders): the
    # reals to the rounding of the terms on both sides plus util.TOL_RUN_ERAW of the largest bin, as the field's two-rank test
    k = min(int(r0['k'][0]), ref.modes_info()['k_E'])
    assert np.all(np.abs(r0['E'] - m['E']) <= 2 * m['N'] * np.ldexp(1.0, -(k + 1)) + TOL_RUN_ERAW * np.max(np.abs(m['E'])))
