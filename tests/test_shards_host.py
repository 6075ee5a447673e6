"""The reference side of test_gpu_shards.py, on the CPU: the oracle's emission sharded over 3, 5 and 8 ranks with the
'constant' and 'fixed_rate' generators, at entry rates where an entry emits up to ten particles per step -- so that the
ownership rule sharding.emission_owner is exercised with several levels per rank -- and the two statements of a segment's
spawn bound (host: nk_spawn_bound, kernel: nk_emit_one's seg_bound) side by side.  test_sharding_gloo.py runs the same
scheme with a real all-reduce at two and four ranks and unscaled entry rates."""
import numpy as np
import pytest

from shard_cases import N0, NSTEPS, SEED, shard_case, oracle_rank, identity, check_owner, assert_union_equals, assert_balanced, \
    spawn_bounds
from util import make_oracle_sim, golden, sub

_SINGLE = {}


def single_run(gen):
    """The unsharded oracle run of 'ttrrp' with generator `gen`: final particles and N_emitted per step; run once."""
    if gen not in _SINGLE:
        ct, pos, mode, occ, counter, scale = shard_case('ttrrp')
        sim = make_oracle_sim(ct, pos, mode, occ, counter, seed=SEED, cap=8 * N0, gen=gen, emit_scale=scale)
        emitted = []
        for _ in range(NSTEPS):
            sim.run_timestep()
            emitted.append(sim.N_emitted)
        n = sim.P.N
        _SINGLE[gen] = (dict(pid=sim.P.pid[:n].copy(), mode=sim.P.mode[:n].copy(), positions=sim.P.pos[:n].copy()), np.array(emitted))
    return _SINGLE[gen]


@pytest.mark.parametrize('gen', [0, 1])
@pytest.mark.parametrize('nranks', [3, 5, 8])
def test_oracle_shards_union_equals_single_run(nranks, gen):
    """Rough walls ('ttrrp': which mode a reflection draws does not depend on the temperature, so trajectories do not
    depend on the tallies a rank sees).  Union of the shards = the single run, ids, modes and positions bit for bit; the
    emission counts add up step by step; every entering particle sits on the rank emission_owner names."""
    ref, emitted_ref = single_run(gen)
    parts, emitted, top = [], np.zeros(NSTEPS, dtype=np.int64), 0
    for r in range(nranks):
        sim = oracle_rank('ttrrp', gen, r, nranks)
        for s in range(NSTEPS):
            sim.run_timestep_sharded(identity)
            emitted[s] += sim.N_emitted
        n = sim.P.N
        parts.append(dict(pid=sim.P.pid[:n].copy(), mode=sim.P.mode[:n].copy(), positions=sim.P.pos[:n].copy()))
        top = max(top, check_owner(parts[-1]['pid'], gen, r, nranks))
    assert np.array_equal(emitted, emitted_ref)
    assert_union_equals(ref, parts)
    assert top >= 9, 'the largest level seen is %d: the case does not reach several levels per rank' % top
    assert_balanced(parts)


def test_check_owner_rejects_a_neighbouring_rank():
    """The checker itself: ids owned by rank 1 of 3 pass for rank 1 and fail for ranks 0 and 2."""
    from nanokappa_amd.sharding import emission_pid
    ids = np.array([emission_pid(rm, lv, st) for rm in range(40) for lv in range(1, 11) for st in range(NSTEPS)
                    if (rm + lv + st) % 3 == 1], dtype=np.uint64)
    assert check_owner(ids, 0, 1, 3) == 10
    for wrong in (0, 2):
        with pytest.raises(AssertionError):
            check_owner(ids, 0, wrong, 3)
    o2o = np.array([((st + 1) << 40) | (r << 32) | i for st in range(NSTEPS) for r in range(2) for i in range(50) if (i + st) % 3 == 1],
                   dtype=np.uint64)
    assert check_owner(o2o, 2, 1, 3) == 0
    with pytest.raises(AssertionError):
        check_owner(o2o, 2, 2, 3)


def test_owned_levels_closed_form():
    """nk_emit_one's closed form for the q-th level a rank owns, counted down from c -- tq = (rank + n - (rm + step) % n) % n,
    top = c - (c + n - tq) % n, level = top - q n -- against the enumeration nk_emit_entry counts with, for every small case."""
    from nanokappa_amd.sharding import emission_owner
    for n in (2, 3, 5, 8):
        for rank in range(n):
            for rm_step in range(n):                       # only (rm + step) % n matters
                for c in range(0, 23):
                    owned = [lv for lv in range(c, 0, -1) if emission_owner(rm_step, lv, 0, n) == rank]
                    tq = (rank + n - rm_step % n) % n
                    top = c - (c + n - tq) % n
                    closed = [top - q * n for q in range(len(owned))]
                    assert closed == owned, (n, rank, rm_step, c)
                    assert top - len(owned) * n < 1        # ... and the next one down is no level any more


def test_spawn_bound_host_and_kernel_sums():
    """nk_spawn_bound (host, sizes the store) divides a segment's whole sum of floor(p) + 1 by the rank count once; the sum
    the sweep's halt criterion uses (nk_emit_one) takes the ceiling entry by entry.  On the golden 'ttp' table dealt over 64
    segments the two part from two ranks on.  DESIGN.md (e) has why the store's slack covers the difference; this pins the
    figures that argument uses and the inequality it rests on: kernel - (host - R) < entries of the segment."""
    ep = sub(golden('setup'), 'velocity')['enter_prob'].reshape(2, -1)
    R, M = ep.shape
    assert (R, M) == (2, 4374)
    got = {n: spawn_bounds(ep, 64, n) for n in (1, 2, 3, 8)}
    assert got == {1: (145, 143), 2: (74, 138), 3: (50, 138), 8: (20, 138)}
    for nseg in (64, 512, 793):
        entries = R * ((M + nseg - 1) // nseg)
        for n in (1, 2, 3, 8):
            for scale in (1.0, shard_case('ttp')[5]):
                host, kernel = spawn_bounds(ep * scale, nseg, n)
                assert kernel >= host - R                       # a sum of ceilings is no less than the ceiling of the sum
                assert kernel - (host - R) < entries
    # the store upload() makes holds 65 536 slots beyond 1.5 N, hence 512 segments or more: 18 entries per segment at most
    assert R * ((M + 511) // 512) == 18
