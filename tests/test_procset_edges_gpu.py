"""GPU: the ProcSet sweep (k_procset_sweep through Random.ProcSetSweep, which returns every seed's statistics) where
the other suites never took it: units of 64 live lanes and up to three units per bucket, event chunks in the tens with
a ragged last chunk and every chunk joint, and the sweep's own uniform restatement of the three sub-policies
(ps_event_uniform) over the parameter grid. The references are the plain-Python one (tests/procset_ref.py over the
oracle's Go generator) and, where every one of 20,000 seeds is compared, the statistics restated over the sweep's own
dump rows, which come from the general per-decision form (k_procset_decide / ps_decide; tests/test_procset_host.py
ties that form to the reference over the whole parameter grid, and the sampled test here ties this sweep to it
directly). Cases and their preconditions: tests/procset_cases.py, tests/test_procset_edges.py. Everything is integer:
every comparison is equality. The chunk counts quoted are chunks(E, S, 256); they hold for any device of 80 compute
units or more."""
import functools

import numpy as np
import pytest

import procset_cases as C
import procset_ref as R
from namazu_amd.explorepolicy import Random
from oracle import oracle as O

pytestmark = pytest.mark.gpu


def policy(name, interval=C.RANGED, use_batch=True, prioritized=3, reset_probability=0.1):
    p = Random()
    p.MinInterval, p.MaxInterval = interval
    p.ProcPolicy = name
    p.PPPMild.UseBatch, p.PPPExtreme.Prioritized, p.PPPDirichlet.ResetProbability = use_batch, prioritized, \
        reset_probability
    ref = C.ref_params(name, use_batch, prioritized, reset_probability)
    return p, O.random_params(interval[0], interval[1], 0.0), ref


def stats_of(r):
    return np.asarray(r.stats).astype(R.STATS_DTYPE)


def same_topk(got, exp):
    return np.array_equal(np.asarray(got).astype(R.TOPK_DTYPE), exp)


# ---- 1. every lane of full units, every seed
def full_units(ctx, name, E, seed0):
    S = C.FULL_S
    sizes = [len(m) for m in C.bucket_members(seed0, S)]
    assert min(sizes) > 64 and max(sizes) <= 128  # a full unit and a partial one in every bucket
    assert C.chunks(E, S, C.N_CU) == {15: (15, 1), 24: (8, 3)}[E]
    tr = C.full_unit_trace(name, E)
    p, _, _ = policy(name)
    r = p.ProcSetSweep(seed0, S, *tr.args(), n_dump=S, k=64, descending=True, ctx=ctx)
    exp = C.stats_from_dump(name, r.delays, r.attrs, tr.n_procs, tr.target)
    got = stats_of(r)
    assert np.array_equal(got, exp)
    assert np.all(got["flags"] == 0)
    assert same_topk(r.topk, R.topk(exp, seed0, 64, True))
    up = p.ProcSetSweep(seed0, S, *tr.args(), k=64, descending=False, ctx=ctx)
    assert np.array_equal(stats_of(up), exp)
    assert same_topk(up.topk, R.topk(exp, seed0, 64, False))
    assert len(set(exp["target_score"].tolist())) > 3  # the top-k has something to order


@pytest.mark.parametrize("E", C.FULL_E)
@pytest.mark.parametrize("name", C.POLICIES)
def test_full_units_every_seed(ctx, name, E):
    """20,000 seeds from 77,000: 77 to 79 seeds per bucket, so every bucket runs one unit of 64 live lanes and one of
    13 to 15. E = 15 is one chunk (plain stores), E = 24 three chunks of 8 (atomics into zeroed statistics). Every
    seed's statistics against the statistics of its own dump row."""
    full_units(ctx, name, E, C.SEED0)


def test_full_units_over_a_range_that_wraps(ctx):
    """The same from seed 2^64 - 10,000: the range wraps past 2^64 in the middle of the sweep."""
    full_units(ctx, "mild", 24, C.WRAP_SEED0)


# ---- 2. three units per bucket, 23 chunks with a ragged tail, against the Python reference on a sample
@functools.lru_cache(maxsize=None)
def sample_reference(name):
    """Computed once per policy and shared; the array is not modified."""
    _, rp, ref = policy(name, prioritized=C.THREE_PRIORITIZED)
    return C.reference_of(C.SEED0, C.sample_indices(), C.three_unit_trace(name), rp, ref)


@pytest.mark.parametrize("name", C.POLICIES)
def test_three_units_per_bucket_and_a_ragged_last_chunk(ctx, name):
    """33,000 seeds from 77,000 over 203 events: 128 to 130 seeds per bucket (226 buckets run a third unit of one or
    two lanes), chunks(203, 33000, 256) = (9, 23) with a last chunk of 5 events. Events of 64, 65 and 512 processes
    (target slot 511), extreme with prioritized = 64, mild with zero-process events at a chunk's last and first
    event. The sample: every seed of two buckets of 129 or 130, the first and the last 64 seeds, and 128 more (513
    seeds)."""
    S, seed0 = C.THREE_S, C.SEED0
    assert C.chunks(C.THREE_E, S, C.N_CU) == (9, 23) and C.THREE_E - 9 * 22 == 5
    sizes = [len(m) for m in C.bucket_members(seed0, S)]
    assert sum(1 for s in sizes if s > 128) >= 200 and max(sizes) <= 130
    sample = np.array(C.sample_indices())
    tr = C.three_unit_trace(name)
    p, _, _ = policy(name, prioritized=C.THREE_PRIORITIZED)
    exp = sample_reference(name)
    if name == "extreme":  # from the reference: slot 511 of the 512-process event is marked for some sampled seed
        _, rp, ref = policy(name, prioritized=C.THREE_PRIORITIZED)
        one = C.Trace(tr.evhash[150:151], tr.evclass[150:151], tr.n_procs[150:151], tr.target[150:151])
        assert (int(one.n_procs[0]), int(one.target[0])) == (512, 511)
        hit = [int(C.reference((seed0 + int(i)) & C.M64, 1, one, rp, ref)["target_score"][0]) > 0 for i in sample]
        assert sum(hit) >= 16
    for desc in (True, False):
        r = p.ProcSetSweep(seed0, S, *tr.args(), k=256, descending=desc, ctx=ctx)
        got = stats_of(r)
        assert np.array_equal(got[sample], exp)
        assert np.all(got["flags"] == 0)
        assert same_topk(r.topk, R.topk(got, seed0, 256, desc))


# ---- 3. chunk joints at a small sweep
@pytest.mark.parametrize("E", sorted(C.JOINT_CHUNKS))
@pytest.mark.parametrize("name", C.POLICIES)
def test_chunk_joints(ctx, name, E):
    """128 seeds, 1 to 6 processes per event, every seed against the reference. (ec, n_chunks) by E:
    15: (15, 1)   16: (8, 2)   17: (9, 2), 9 + 8   31: (11, 3), 11 + 11 + 9   32: (8, 4)   33: (9, 4), 9 + 9 + 9 + 6
    65: (9, 8), seven of 9 and one of 2."""
    assert C.chunks(E, C.JOINT_S, C.N_CU) == C.JOINT_CHUNKS[E]
    tr = C.joint_trace(E)
    assert len(tr) == E and 1 <= tr.n_procs.min() and tr.n_procs.max() <= 6
    p, rp, ref = policy(name)
    exp = C.reference(C.JOINT_SEED0, C.JOINT_S, tr, rp, ref)
    r = p.ProcSetSweep(C.JOINT_SEED0, C.JOINT_S, *tr.args(), k=8, ctx=ctx)
    assert np.array_equal(stats_of(r), exp)
    assert same_topk(r.topk, R.topk(exp, C.JOINT_SEED0, 8, True))


# ---- 4. the uniform form over the parameter grid: no dump, so only the statistics path runs
def grid_cell(ctx, name, interval, tr, hits=None, **kw):
    """-> (the sweep's statistics, the reference's), asserted equal, for GRID_S seeds over one trace."""
    S, seed0 = C.GRID_S, C.GRID_SEED0
    assert C.chunks(len(tr), S, C.N_CU)[1] == 1
    p, rp, ref = policy(name, interval=C.INTERVALS[interval], **kw)
    exp = C.reference(seed0, S, tr, rp, ref, hits=hits)
    got = stats_of(p.ProcSetSweep(seed0, S, *tr.args(), ctx=ctx))
    assert np.array_equal(got, exp), (name, interval, kw)
    return got, exp


@pytest.mark.parametrize("interval", sorted(C.INTERVALS))
@pytest.mark.parametrize("prioritized", C.EXTREME_PRIORITIZED)
def test_extreme_uniform_form(ctx, prioritized, interval):
    """prioritized <= 0, 1, 64, 256 over n_procs 1 .. 512 with targets at bit 31 of a mark word, bit 0 of the next
    and slot 511; then the same trace without targets. With prioritized <= 0 the trace also has an event of no
    process. At 256 the events of 1, 2 and 3 processes have every slot marked (checked on those events alone)."""
    tr = dict(C.extreme_cells())[prioritized]
    hits = np.zeros((C.GRID_S, len(tr)), np.int64)
    got, exp = grid_cell(ctx, "extreme", interval, tr, hits=hits, prioritized=prioritized)
    n = tr.n_procs.tolist()
    if prioritized <= 0:
        assert not hits.any() and np.all(exp["n_special"] == 0) and np.all(exp["score_sum"] == 0)
    else:  # from the reference alone: the targets do hit marked slots
        assert np.count_nonzero(hits) >= 16
        assert np.all(hits[:, 0] > 0)  # one process: always marked
    if prioritized >= 64:
        big = [e for e in range(len(n)) if n[e] >= 31]
        assert np.count_nonzero(hits[:, big]) >= 16 and all(hits[:, e].any() for e in big)
        assert len(set(hits[:, big].ravel().tolist())) == 11  # 0 and every priority
    none, exp_none = grid_cell(ctx, "extreme", interval, tr.without_targets(), prioritized=prioritized)
    assert np.all(exp_none["target_score"] == 0)
    assert np.array_equal(none["score_sum"], got["score_sum"]) and np.array_equal(none["n_special"], got["n_special"])
    if prioritized == 256:
        small = C.Trace(tr.evhash[:3], tr.evclass[:3], tr.n_procs[:3], tr.target[:3])
        assert small.n_procs.tolist() == [1, 2, 3]
        got3, _ = grid_cell(ctx, "extreme", interval, small, prioritized=prioritized)
        assert np.all(got3["n_special"] == 1 + 2 + 3)


@pytest.mark.parametrize("interval", sorted(C.INTERVALS))
@pytest.mark.parametrize("reset_probability,threshold", C.DIRICHLET_RESET)
def test_dirichlet_uniform_form(ctx, reset_probability, threshold, interval):
    """Thresholds 0, 1, 999 and 1000 of Intn(999) < threshold: never, a draw of 0 only, and twice always (Intn(999)
    is at most 998)."""
    tr = C.grid_trace()
    hits = np.zeros((C.GRID_S, len(tr)), np.int64)
    got, exp = grid_cell(ctx, "dirichlet", interval, tr, hits=hits, reset_probability=reset_probability)
    total = int(tr.n_procs.sum())
    if threshold == 0:
        assert np.all(got["score_sum"] == 0) and np.all(got["target_score"] == 0)
    if threshold >= 999:
        assert np.all(got["score_sum"] == total) and np.all(got["target_score"] == len(tr))
    if threshold == 1:  # from the reference: some draw is 0, most are not
        assert 16 <= np.count_nonzero(exp["score_sum"]) and exp["score_sum"].max() < 20
    assert np.array_equal(got["n_special"].astype(np.int64), got["score_sum"])


@pytest.mark.parametrize("interval", sorted(C.INTERVALS))
def test_mild_uniform_form(ctx, interval):
    """n = 0, 1, 512 with targets 0 and 511; use_batch changes the attrs' policy only, never the statistics."""
    tr = C.mild_grid_trace()
    hits = np.zeros((C.GRID_S, len(tr)), np.int64)
    a, exp = grid_cell(ctx, "mild", interval, tr, hits=hits, use_batch=False)
    b, _ = grid_cell(ctx, "mild", interval, tr, use_batch=True)
    assert np.array_equal(a, b)
    assert not hits[:, 0].any() and all(len(set(hits[:, e].tolist())) > 20 for e in (1, 2, 3))
