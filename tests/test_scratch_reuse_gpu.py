"""GPU: the context's scratch slots across calls. Every other GPU test calls one feature per context state; here one
context (the session's, never closed in between) runs the sequences in which a slot assignment, a slot that grows
again after another user, or a zero-count field of a scratch layout (csrc/scratch_layout.h) could go wrong:

  1. two host forms that share a slot, one after the other, small - large - small;
  2. the three groups of slots that are live inside one call;
  3. calls whose layouts have fields of count zero.

Every output is compared exactly with the matching host entry point or with the references of tests/*_ref.py and
the C oracle. Nothing here depends on a rate."""
import ctypes

import numpy as np
import pytest

import contrast_ref as C
import delivery_ref as DR
import moves_cases as MC
import order_ref as OR
import procset_ref as PR
import sig_ref as SR
import target_ref as TR
from namazu_amd import _lib
from namazu_amd import historystorage as hs
from namazu_amd.explorepolicy import Random, Replayable
from oracle import oracle as O

pytestmark = pytest.mark.gpu

MS = 1_000_000
M = 100 * MS
# two events: the smallest trace the sweeps take with something to order
HINTS = ["hint-entity-0-0", "hint-entity-1-1"]
ARRIVAL = np.array([0, 5 * MS], np.int64)
SYM = np.array([11, 22], np.uint64)
CONS = [(1, 0, MS)]
TARGET_POS = np.array([1, 0], np.uint32)
COUNTS = [(1, 300, 1), (300, 1, 300)]  # the shared slot grows, is reused small, and grows again -- and the mirror


def replayable(m=M):
    p = Replayable()
    p.MaxInterval = m
    return p


def seeds_of(n, lo=0):
    return [str(lo + i) for i in range(n)]


def order_sweep(ctx, n, decimal=False):
    seeds = seeds_of(n, 7)
    kw = dict(seed_lo=7, n_seeds=n) if decimal else dict(seeds=seeds)
    r = replayable().OrderSweep(HINTS, ARRIVAL, CONS, k=1, ctx=ctx, **kw)
    st, _ = OR.host_order(seeds, HINTS, ARRIVAL, CONS, M)
    assert OR.same(r.stats, st.astype(OR.STATS_DTYPE))
    vals = np.arange(7, 7 + n, dtype=np.uint64) if decimal else np.arange(n, dtype=np.uint64)
    assert OR.same(r.topk, OR.topk(st.astype(OR.STATS_DTYPE), vals, 1))


def replayable_sweep(ctx, n):
    seeds = seeds_of(n, 3)
    r = replayable().Sweep(seeds, HINTS, n_dump=1, k=1, ctx=ctx)
    so, sb = O.to_csr(seeds)
    ho, hb = O.to_csr(HINTS)
    st, dl = O.replayable_sweep(so, sb, ho, hb, M, n_dump=1)
    assert np.array_equal(r.stats, st) and np.array_equal(r.delays, dl)
    assert np.array_equal(r.topk, O.topk_from_stats(st, 0, 1))


def target_sweep(ctx, n, decimal=False):
    seeds = seeds_of(n, 5)
    kw = dict(seed_lo=5, n_seeds=n) if decimal else dict(seeds=seeds)
    r = replayable().NearestOrders(HINTS, ARRIVAL, target_pos=TARGET_POS, k=1, ctx=ctx, **kw)
    st, n_counted, n_pairs = TR.host_target(seeds, HINTS, ARRIVAL, None, TARGET_POS, M)
    assert r.stats.tobytes() == st.tobytes()
    assert (r.n_counted, r.n_pairs) == (n_counted, n_pairs)
    vals = np.arange(5, 5 + n, dtype=np.uint64) if decimal else np.arange(n, dtype=np.uint64)
    assert np.array_equal(r.topk.astype(TR.TOPK_DTYPE), TR.topk(st.astype(TR.STATS_DTYPE), n_pairs, vals, 1, "pairs"))


def delivery_classes(st):
    """first_equal, class_rep and n_classes of host-form stats, by tests/sig_ref.py."""
    fe = SR.first_equal(list(zip(st["sig_lo"].tolist(), st["sig_hi"].tolist())))
    return fe, SR.class_rep(fe, st["min_gap_ns"].tolist()), SR.n_classes(fe)


def delivery_sweep(ctx, seeds, hints=HINTS, arrival=ARRIVAL, sym=SYM, decimal_lo=None):
    kw = dict(seeds=seeds) if decimal_lo is None else dict(seed_lo=decimal_lo, n_seeds=len(seeds))
    r = replayable().DeliveryOrders(hints, arrival, sym, ctx=ctx, **kw)
    st = DR.host_delivery(seeds, hints, arrival, sym, None, M)[0]
    assert r.stats.tobytes() == st.tobytes()
    fe, rep, nc = delivery_classes(st)
    assert r.first_equal.tolist() == fe and r.class_rep.tolist() == rep and r.n_classes == nc
    return fe


@pytest.mark.parametrize("counts", COUNTS)
def test_order_and_replayable_sweeps_share_a_slot(ctx, counts):
    order_sweep(ctx, counts[0])
    replayable_sweep(ctx, counts[1])
    order_sweep(ctx, counts[2])


@pytest.mark.parametrize("counts", COUNTS)
def test_target_and_delivery_sweeps_share_a_slot(ctx, counts):
    target_sweep(ctx, counts[0])
    delivery_sweep(ctx, seeds_of(counts[1], 9))
    target_sweep(ctx, counts[2])


# ---- the random and the ProcSetEvent decisions and sweeps
RNG = np.random.default_rng(77)
EVHASH = RNG.integers(0, 2**64, size=40, dtype=np.uint64)
EVCLASS = (np.arange(40) % 2).astype(np.uint8)
N_PROCS = (np.arange(40) % 5 + 1).astype(np.uint32)
INTERVAL = (30 * MS, 100 * MS)


def random_policy(seed=1234):
    p = Random()
    p.MinInterval, p.MaxInterval, p.FaultActionProbability = INTERVAL[0], INTERVAL[1], 0.1
    p.Seed = seed
    return p


def procset_policy(seed=1234):
    p = Random()
    p.MinInterval, p.MaxInterval = INTERVAL
    p.ProcPolicy = "mild"
    p.Seed = seed
    return p, O.random_params(INTERVAL[0], INTERVAL[1], 0.0), PR.Params(0, True, 3, 0.1)


def random_decide(ctx, E):
    L = _lib.load()
    p = random_policy()
    rp = p.params()
    eh, ec = np.ascontiguousarray(EVHASH[:E]), np.ascontiguousarray((EVCLASS[:E] | 2).astype(np.uint8))
    d, f = np.zeros(E, np.int64), np.zeros(E, np.uint8)
    hd, hf = np.zeros(E, np.int64), np.zeros(E, np.uint8)
    _lib.check(L.nmz_random_decide(ctx.handle, int(p.Seed), _lib.ptr(eh), _lib.ptr(ec), E, ctypes.byref(rp),
                                   _lib.ptr(d), _lib.ptr(f)))
    _lib.check(L.nmz_random_decide_host(int(p.Seed), _lib.ptr(eh), _lib.ptr(ec), E, ctypes.byref(rp), _lib.ptr(hd),
                                        _lib.ptr(hf)))
    assert np.array_equal(d, hd) and np.array_equal(f, hf)


def procset_decide(ctx, E):
    L = _lib.load()
    p, _, _ = procset_policy()
    rp, pp = p.params(), p.procset_params()
    eh, ec, npr = (np.ascontiguousarray(EVHASH[:E]), np.ascontiguousarray(EVCLASS[:E]),
                   np.ascontiguousarray(N_PROCS[:E]))
    total = int(npr.sum())
    out = []
    for host in (False, True):
        d, a = np.zeros(E, np.int64), np.zeros(total, _lib.PROC_ATTR_DTYPE)
        if host:
            rc = L.nmz_procset_decide_host(int(p.Seed), _lib.ptr(eh), _lib.ptr(ec), _lib.ptr(npr), E,
                                           ctypes.byref(rp), ctypes.byref(pp), _lib.ptr(d), _lib.ptr(a))
        else:
            rc = L.nmz_procset_decide(ctx.handle, int(p.Seed), _lib.ptr(eh), _lib.ptr(ec), _lib.ptr(npr), E,
                                      ctypes.byref(rp), ctypes.byref(pp), _lib.ptr(d), _lib.ptr(a))
        _lib.check(rc)
        out.append((d, a))
    assert np.array_equal(out[0][0], out[1][0]) and out[0][1].tobytes() == out[1][1].tobytes()


@pytest.mark.parametrize("events", [(1, 40, 1), (40, 1, 40)])
def test_random_and_procset_decisions_share_a_slot(ctx, events):
    random_decide(ctx, events[0])
    procset_decide(ctx, events[1])
    random_decide(ctx, events[2])


def random_sweep(ctx, n):
    p = random_policy()
    eh, ec = EVHASH[:2], (EVCLASS[:2] | 2).astype(np.uint8)
    r = p.Sweep(7, n, eh, ec, n_dump=1, k=1, ctx=ctx)
    st, dl, fl = O.random_sweep(7, n, eh, ec, O.random_params(INTERVAL[0], INTERVAL[1], 0.1), n_dump=1)
    assert np.array_equal(r.stats, st) and np.array_equal(r.delays, dl) and np.array_equal(r.faults, fl)
    assert np.array_equal(r.topk, O.topk_from_stats(st, 7, 1))


def procset_sweep(ctx, n):
    p, rp, ref = procset_policy()
    eh, ec, npr = EVHASH[:2], EVCLASS[:2], N_PROCS[:2]
    target = np.array([0, 1], np.uint32)
    r = p.ProcSetSweep(7, n, eh, ec, npr, target, n_dump=1, k=1, ctx=ctx)
    st, dl, at, _ = PR.sweep(7, n, eh, ec, npr, target, rp, ref, n_dump=1)
    assert np.array_equal(np.asarray(r.stats).astype(PR.STATS_DTYPE), st)
    assert np.array_equal(r.delays, dl) and np.array_equal(np.asarray(r.attrs).astype(PR.ATTR_DTYPE), at)
    assert np.array_equal(np.asarray(r.topk).astype(PR.TOPK_DTYPE), PR.topk(st, 7, 1, True))


@pytest.mark.parametrize("counts", COUNTS)
def test_random_and_procset_sweeps_share_a_slot(ctx, counts):
    random_sweep(ctx, counts[0])
    procset_sweep(ctx, counts[1])
    random_sweep(ctx, counts[2])


# ---- slots that are live together inside one call
def test_contrast_from_runs_holds_three_buffers(ctx):
    """nmz_order_contrast_runs: the host form's slot, contrast_run's slot and the match call's pool buffer at once.
    3 runs, 4 events, k = 2."""
    sym = np.array([5, 6, 7, 8], np.uint64)
    arrival = np.arange(4, dtype=np.int64) * MS
    runs = [np.array(r, np.uint64) for r in ([5, 6, 7, 8], [6, 5, 8, 7], [8, 7, 6])]  # the last run lacks an event
    failed = np.array([1, 0, 1], np.uint8)
    res = hs.order_contrast_runs(sym, arrival, runs, failed, k=2, want_counts=True, ctx=ctx)
    pos = hs.run_positions(sym, arrival, runs)  # the host matching (match_target)
    F, P = C.counts(pos, failed)
    exp, n_positive = C.ranked(F, P, failed, 2)
    assert np.array_equal(res.counts["n_fail_with"], F) and np.array_equal(res.counts["n_pass_with"], P)
    assert (res.n_fail, res.n_pass, res.n_positive) == (2, 1, n_positive) and n_positive >= 2
    assert res.pairs.tobytes() == exp.astype(_lib.ORDER_PAIR_DTYPE).tobytes()
    for p in res.pairs:  # and the host entry point, pair by pair
        one, _, _ = hs.order_pair(pos, failed, int(p["before"]), int(p["after"]))
        assert one.tobytes() == p.tobytes()


def test_delivery_sweep_with_classes_holds_three_slots(ctx):
    """The delivery host form with first_equal, class_rep and n_classes: its own slot, the class builder's, the sort's
    and the rank-key table. 5 seeds over 3 events, two of them in one class."""
    hints = HINTS + ["hint-entity-0-2"]
    arrival = np.array([0, MS, 2 * MS], np.int64)
    sym = np.array([11, 22, 33], np.uint64)
    # from the host form alone: two seeds that deliver one order, three that deliver three others
    cand = seeds_of(60)
    st = DR.host_delivery(cand, hints, arrival, sym, None, M)[0]
    by_sig = {}
    for s, rec in zip(cand, st):
        by_sig.setdefault((int(rec["sig_lo"]), int(rec["sig_hi"])), []).append(s)
    groups = sorted(by_sig.values(), key=len, reverse=True)
    assert len(groups) >= 4 and len(groups[0]) >= 2, "degenerate input: the candidates do not give four orders"
    seeds = [groups[1][0], groups[0][0], groups[2][0], groups[0][1], groups[3][0]]
    fe = delivery_sweep(ctx, seeds, hints, arrival, sym)
    assert fe == [0, 1, 2, 1, 4]  # the shared class is there


def test_bitvector_query_that_spills_holds_three_slots(ctx):
    """nmz_ed_plan_query_knn on a bit-parallel plan with a query longer than every stored trace: the lists' slot, the
    bit-vector form's and the generic kernel's. 4 stored traces of length <= 8, band 8, two queries."""
    stored = [np.array(t, np.uint64) for t in ([1, 2, 3, 4, 5, 6, 7, 8], [1, 2, 3, 4], [8, 7, 6, 5, 4], [2, 3, 4, 5, 6, 7])]
    ts = hs.TraceSet(stored)
    qs = [np.array([1, 2, 3, 5], np.uint64), np.array([1, 2, 3, 4, 5, 6, 7, 8, 9, 9], np.uint64)]
    L = _lib.load()
    idx = hs.SimilarityIndex(ts, 8, ctx=ctx)
    tot, cnt = ctypes.c_double(), ctypes.c_uint64()
    try:
        assert idx.bitparallel
        _lib.check(L.nmz_timing_enable(ctx.handle, 1))
        _lib.check(L.nmz_timing_read(ctx.handle, b"ed_query_generic", ctypes.byref(tot), ctypes.byref(cnt), 1))
        ids, ds = idx.query(qs, 3)
        _lib.check(L.nmz_timing_read(ctx.handle, b"ed_query_generic", ctypes.byref(tot), ctypes.byref(cnt), 1))
    finally:
        L.nmz_timing_enable(ctx.handle, 0)
        idx.close()
    assert cnt.value >= 1, "the long query did not reach the generic kernel"
    n = len(stored)
    pairs = np.stack([np.zeros(n, np.uint32), np.arange(1, n + 1, dtype=np.uint32)], 1)
    for r, q in enumerate(qs):
        both = hs.TraceSet([q] + stored)
        d = np.minimum(O.ed_pairs(both.off, both.sym, pairs, 8), 9)  # beyond the band: band + 1
        order = np.lexsort((np.arange(n), d))[:3]
        assert ds[r].tolist() == d[order].tolist() and ids[r].tolist() == order.tolist(), r


# ---- zero-count fields
MOVE_TRACES = tuple(np.array(t, np.uint64) for t in ([1, 2, 3, 4], [2, 1, 3, 4], [1, 3, 4, 2]))
MOVE_PAIRS = np.array([(0, 1), (0, 2), (1, 2)], np.uint32)
MOVE_BAND = 4


def test_move_profile_without_a_table_and_without_partners(ctx):
    ts = hs.TraceSet(list(MOVE_TRACES))
    eh = MC.host_scripts(MOVE_TRACES, MOVE_PAIRS, MOVE_BAND)
    none = np.zeros(0, np.uint64)
    want = hs.move_profile_of(ts, MOVE_PAIRS, eh, usym=none, want_partner=True, host=True)
    assert int(want.info["n_ops"]) > 0 and int(want.info["n_unknown"]) > 0
    got = hs.move_profile_of(ts, MOVE_PAIRS, eh, ctx=ctx, usym=none, want_partner=True)  # n_usym = 0
    assert got.info.tobytes() == want.info.tobytes() and np.array_equal(got.partner, want.partner)
    plain = hs.move_profile_of(ts, MOVE_PAIRS, eh, ctx=ctx)  # partner = NULL, every symbol
    full = hs.move_profile_of(ts, MOVE_PAIRS, eh, want_partner=True, host=True)
    assert plain.counts.tobytes() == full.counts.tobytes() and plain.info.tobytes() == full.info.tobytes()


def test_diff_profile_without_dist(ctx):
    ts = hs.TraceSet(list(MOVE_TRACES))
    want = hs.move_profile_of(ts, MOVE_PAIRS, MC.host_scripts(MOVE_TRACES, MOVE_PAIRS, MOVE_BAND), host=True)
    usym = want.symbols
    counts = np.zeros(len(usym), _lib.MOVE_COUNTS_DTYPE)
    info = np.zeros(1, _lib.MOVE_INFO_DTYPE)
    _lib.check(_lib.load().nmz_ed_diff_profile(ctx.handle, _lib.ptr(ts.off), _lib.ptr(ts.sym), len(ts),
                                               _lib.ptr(MOVE_PAIRS), len(MOVE_PAIRS), MOVE_BAND, _lib.ptr(usym),
                                               len(usym), None, _lib.ptr(counts), _lib.ptr(info)))  # dist = NULL
    assert counts.tobytes() == want.counts.tobytes() and info[0].tobytes() == want.info.tobytes()


def test_contrast_without_counts_and_without_pairs(ctx):
    pos, failed, F, P = C.case(5, 4)
    res = hs.order_contrast(pos, failed, k=0, ctx=ctx)  # counts = NULL, k = 0
    assert res.counts is None and len(res.pairs) == 0
    n_fail = int(np.count_nonzero(failed))
    n_positive = int(np.count_nonzero(C.scores(F, P, failed) > 0))
    assert n_positive > 0
    assert (res.n_fail, res.n_pass, res.n_positive) == (n_fail, len(failed) - n_fail, n_positive)


@pytest.mark.parametrize("n", [1, 300])
def test_decimal_sweeps_upload_no_seed_bytes(ctx, n):
    target_sweep(ctx, n, decimal=True)
    order_sweep(ctx, n, decimal=True)
    delivery_sweep(ctx, seeds_of(n, 9), decimal_lo=9)


def test_unique_traces_without_entities_and_with_an_empty_trace(ctx):
    for traces in ([[1, 2, 3], [3, 2, 1], [1, 2, 3]], [[4, 5], [], [4, 5]], [[], [6], []]):
        ts = hs.TraceSet([np.array(t, np.uint64) for t in traces])
        got = hs.first_equal(ts, ctx=ctx)  # entity = NULL
        assert got.tolist() == SR.first_equal([SR.signature(t) for t in traces])
        assert got.tolist() == [traces.index(t) for t in traces]
