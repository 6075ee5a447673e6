"""The engine's rank-dependent code at 3, 5 and 8 ranks on ONE GPU: contexts with a rank and a rank count but no communicator
(NK_COMM_DRYRUN, so every tally stays the rank's own), one after another on device 0.  The emission is scaled so that an entry
emits up to ten particles per step: the level ownership of nk_emit_one / nk_emit_entry, k_emit_one_to_one's owner rule, the
'fixed_rate' dice and the large-mesh queue path all see values they never see at two ranks with two levels per entry
(test_gpu_parity.py::test_two_rank_sharding_on_one_gpu).  Shapes and helpers: shard_cases.py; the oracle's side of the same
scheme alone: test_shards_host.py.  The runs with a communicator need as many GPUs as ranks: test_gpu_multirank.py."""
import numpy as np
import pytest

from shard_cases import N0, NSTEPS, SEED, GEN_NAMES, shard_case, oracle_rank, identity, check_owner, assert_union_equals, \
    assert_balanced, spawn_bounds
from util import make_engine, allclose, rel_err, same_event_rule, oracle_row, assert_rows, TOL_X, TOL_OCC

pytestmark = pytest.mark.gpu

DRY = bytes(128)                  # the unique id of a communicator that is never made

_SINGLE = {}


def single_rank_run(case, gen):
    """The engine's unsharded run of the case: tally rows, final particles, halts.  Run once per (case, generator), shared
    by the tests and never modified."""
    if (case, gen) not in _SINGLE:
        ct, pos, mode, occ, counter, scale = shard_case(case)
        eng = make_engine(ct, pos, mode, occ, counter, seed=SEED, gen=gen, emit_scale=scale)
        t = eng.step(NSTEPS)
        rows = {k: np.array(t[k], copy=True) for k in ('N_emitted', 'N_leaving', 'N_sv')}
        p = eng.download()
        tm = eng.timing()
        eng.close()
        for a in list(rows.values()) + [p['pid'], p['mode'], p['positions']]:
            a.setflags(write=False)
        _SINGLE[(case, gen)] = (rows, p, tm)
    return _SINGLE[(case, gen)]


def rank_engine(case, gen, rank, nranks):
    from nanokappa_amd.sharding import shard_range
    ct, pos, mode, occ, counter, scale = shard_case(case)
    lo, hi = shard_range(N0, rank, nranks)
    return make_engine(ct, pos[lo:hi], mode[lo:hi], occ[lo:hi], counter, seed=SEED, gen=gen, emit_scale=scale, pid_offset=lo,
                       comm=(DRY, rank, nranks))


def segment_bounds(eng, case, nranks):
    """(segments, (host, kernel)) of the engine's store: the two spawn bounds of shard_cases.spawn_bounds on the deal of the modes
    that this store uses; for the record (profiles/shard_parity_margins.txt), nothing is asserted on them."""
    from nanokappa_amd.engine import NkError
    ct, scale = shard_case(case)[0], shard_case(case)[5]
    try:
        seg, nseg = eng.mode_segments()
    except NkError:                              # a store without partitioned modes
        return 0, None
    return nseg, spawn_bounds(ct['enter_prob'] * scale, nseg, nranks, seg)


def run_shards(case, gen, nranks, monkeypatch, steps=NSTEPS):
    """Every rank of the case in turn (one live context at a time): rows summed over the ranks, particles, timing per rank."""
    monkeypatch.setenv('NK_COMM_DRYRUN', '1')
    rows, parts, tms = None, [], []
    for r in range(nranks):
        e = rank_engine(case, gen, r, nranks)
        tm0 = e.timing()
        t = e.step(steps)                        # must not raise: a halt is served by growing the store
        tr = {k: np.array(t[k], dtype=np.float64) for k in ('N_emitted', 'N_leaving', 'N_sv')}
        rows = tr if rows is None else {k: rows[k] + tr[k] for k in tr}
        parts.append(e.download())
        tm = e.timing()
        tm['slots0'] = tm0['slots']
        tm['nseg'], tm['bounds'] = segment_bounds(e, case, nranks)
        tms.append(tm)
        e.close()
    return rows, parts, tms


def report(what, case, gen, nranks, tms, parts, top):
    print('\nshards %s: %s %s %d ranks: halts %s regrows %s slots %s -> %s sizes %s top level %d; rank 0: %d segments, spawn bound (host, kernel) %s'
          % (what, case, GEN_NAMES[gen], nranks, [t['halts'] for t in tms], [t['regrows'] for t in tms], [t['slots0'] for t in tms],
             [t['slots'] for t in tms], [q['pid'].shape[0] for q in parts], top, tms[0]['nseg'], tms[0]['bounds']))


UNION_CASES = [('ttp', g, n) for g in (0, 1) for n in (3, 5, 8)] + [('ttrrp', 0, 3), ('ttrrp', 0, 8), ('wire72', 1, 5)]


@pytest.mark.parametrize('case,gen,nranks', UNION_CASES)
def test_union_of_shards_equals_single_rank(case, gen, nranks, monkeypatch):
    """Trajectories do not depend on the temperatures (rough walls: which mode a diffuse reflection draws does not, only its
    occupation), so the shards together must hold exactly the single-rank run's particles, their counts must add up to its
    rows step by step, every entering particle must sit on the rank sharding.emission_owner names -- two ranks creating the
    same particle, or none, fails the first; a rank creating another's, the last -- and no rank may stop to grow a store
    that the single-rank run did not have to grow (nk_spawn_bound against the sweep's halt criterion)."""
    rows1, p1, tm1 = single_rank_run(case, gen)
    rows, parts, tms = run_shards(case, gen, nranks, monkeypatch)
    top = max(check_owner(q['pid'], gen, r, nranks) for r, q in enumerate(parts))
    report('union', case, gen, nranks, tms, parts, top)
    print('single rank: halts %d slots %d' % (tm1['halts'], tm1['slots']))
    assert_union_equals(p1, parts)
    for k in ('N_emitted', 'N_leaving', 'N_sv'):
        assert np.array_equal(rows[k], rows1[k]), '%s: the ranks do not add up to the single-rank run' % k
    assert top >= 9, 'the largest level seen is %d: the case does not reach several levels per rank' % top
    assert_balanced(parts)
    if tm1['halts'] == 0:
        assert [t['halts'] for t in tms] == [0] * nranks, 'a rank halted where the single-rank run did not'


PARITY_CASES = [('ttp', g, n) for g in (0, 1, 2) for n in (3, 8)] + [('ttrrp', 2, 5)]


@pytest.mark.parametrize('case,gen,nranks', PARITY_CASES)
def test_rank_against_the_oracles_same_rank(case, gen, nranks, monkeypatch):
    """Engine context (rank, nranks, no communicator) against the oracle with the same rank and an all-reduce that sums
    nothing: both tally their own shard only, so the temperatures and occupations are comparable as well, and 'one_to_one'
    can run sharded -- both feed their own N_leaving into the next step's emission, both keep candidate i when
    (i + step) % nranks is their rank, both start from first_n_leaving.  Ranks 0, 1 and the last; rows step by step, then
    particle by particle."""
    monkeypatch.setenv('NK_COMM_DRYRUN', '1')
    top = 0
    for r in sorted({0, 1, nranks - 1}):
        sim = oracle_rank(case, gen, r, nranks)
        eng = rank_engine(case, gen, r, nranks)
        same_event_rule(eng, sim)
        t = eng.step(NSTEPS)
        for s in range(NSTEPS):
            sim.run_timestep_sharded(identity)
            assert_rows(t, s, oracle_row(sim))
            if gen == 2:
                assert t['N_emitted'][s] > 0, "rank %d's 'one_to_one' reservoirs emit nothing at step %d: the case checks nothing there" % (r, s)
                if s > 0:                       # of the candidates 0 .. N_leaving[s - 1] of each reservoir, those with (i + s) % nranks == r
                    mine = sum(int(np.sum((np.arange(int(nl)) + s) % nranks == r)) for nl in t['N_leaving'][s - 1])
                    assert t['N_emitted'][s] == mine
        p = eng.download()
        eng.close()
        n = sim.P.N
        top = max(top, check_owner(p['pid'], gen, r, nranks))
        o1, o2 = np.argsort(p['pid']), np.argsort(sim.P.pid[:n])
        assert p['pid'].shape[0] == n
        assert np.array_equal(p['pid'][o1], sim.P.pid[:n][o2])
        assert np.array_equal(p['mode'][o1], sim.P.mode[:n][o2])
        assert allclose(p['positions'][o1], sim.P.pos[:n][o2], rtol=0, atol=TOL_X)
        assert rel_err(p['occupation'][o1], sim.P.occ[:n][o2], bound=TOL_OCC) < TOL_OCC
    if gen != 2:
        assert top >= 9, 'the largest level seen is %d: the case does not reach several levels per rank' % top


def test_five_rank_shards_grow_with_rough_walls(monkeypatch):
    """test_two_rank_shards_grow_with_rough_walls at five ranks and up to ten particles per entry: stores with hardly any
    head room (NK_TIGHT_STORE) that the entering particles outgrow within the twelve steps.  Some rank must halt and grow,
    none may give up ('keeps filling up': step() would raise), and the union is still the single-rank run."""
    rows1, p1, tm1 = single_rank_run('ttrrp', 0)
    monkeypatch.setenv('NK_TIGHT_STORE', '1')
    rows, parts, tms = run_shards('ttrrp', 0, 5, monkeypatch)
    top = max(check_owner(q['pid'], 0, r, 5) for r, q in enumerate(parts))
    report('tight', 'ttrrp', 0, 5, tms, parts, top)
    assert max(t['halts'] for t in tms) > 0 and max(t['regrows'] for t in tms) > 0, 'no store had to grow: the case checks nothing'
    assert_union_equals(p1, parts)
    for k in ('N_emitted', 'N_leaving', 'N_sv'):
        assert np.array_equal(rows[k], rows1[k])
    assert top >= 9
