"""GPU: nmz_order_contrast against the numpy restatement (tests/contrast_ref.py): full counts, listed pairs (all
seven fields, sentinels included) and info at the tile and run-chunk edges, the d_counts == NULL form, the packed
counter's edge at 65,535 runs, one full-size case, antisymmetry on all-present runs, the loop from a generated
storage to a seed that delivers the planted order, and run-to-run determinism."""
import json
import os

import numpy as np
import pytest

import contrast_ref as C
from namazu_amd import _lib, historystorage as hs, replay
from namazu_amd.explorepolicy import Replayable
from test_contrast_host import GPU_CASES, pair_tuple
from test_visualize import write_store, zk_store_traces

pytestmark = pytest.mark.gpu

SMALL = [c for c in GPU_CASES if c[0] <= 257]


def check_counts(got, F, P):
    assert np.array_equal(got["n_fail_with"], F)
    assert np.array_equal(got["n_pass_with"], P)


def check_listed(res, F, P, failed, k):
    exp, n_positive = C.ranked(F, P, failed, k)
    assert res.n_positive == n_positive
    assert (res.n_fail, res.n_pass) == (int(failed.sum()), len(failed) - int(failed.sum()))
    assert res.pairs.dtype == _lib.ORDER_PAIR_DTYPE and len(res.pairs) == k
    assert [pair_tuple(p) for p in res.pairs] == [pair_tuple(p) for p in exp]


@pytest.mark.parametrize("E,R", SMALL)
def test_counts_pairs_and_info(ctx, E, R):
    pos, failed, F, P = C.case(E, R)
    for k in (1, 64, 256):
        res = hs.order_contrast(pos, failed, k=k, want_counts=True, ctx=ctx)
        check_counts(res.counts, F, P)
        check_listed(res, F, P, failed, k)
    if E == 1:
        assert res.n_positive == 0 and int(res.pairs[0]["before"]) == C.NONE
    # the hot form: no counts, the same list
    hot = hs.order_contrast(pos, failed, k=64, ctx=ctx)
    assert hot.counts is None
    check_listed(hot, F, P, failed, 64)


def test_many_tiles_with_a_ragged_edge(ctx):
    """E = 2,049: one event past a multiple of both tile edges (64 columns, 32 rows), 2,145 workgroups, and with
    three runs some waves of a workgroup get no run at all."""
    pos, failed, F, P = C.case(2049, 3)
    res = hs.order_contrast(pos, failed, k=64, want_counts=True, ctx=ctx)
    check_counts(res.counts, F, P)
    check_listed(res, F, P, failed, 64)


@pytest.mark.parametrize("invert", [False, True])
def test_the_packed_counter_at_65535_runs(ctx, invert):
    """One run of one label and 65,534 of the other, all agreeing on event 0 ahead of event 1: a count of 65,534 in
    one half of the packed counter and nothing leaking into the other half."""
    E, R = 8, 65535
    rng = np.random.default_rng(8)
    pos = np.argsort(rng.random((R, E)), axis=1).astype(np.uint32) * 2 + 2
    pos[:, 0] = 0  # event 0 first in every run, so (0, 1) is ordered one way by all of them
    pos[rng.random((R, E)) < 0.1] = C.NONE
    pos[:, 0] = 0
    pos[pos[:, 1] == C.NONE, 1] = 1
    failed = np.zeros(R, np.uint8)
    failed[12345] = 1
    if invert:
        failed ^= 1
    F, P = C.counts(pos, failed)
    assert (P if not invert else F)[0, 1] == 65534 and (F if not invert else P)[0, 1] == 1
    res = hs.order_contrast(pos, failed, k=64, want_counts=True, ctx=ctx)
    check_counts(res.counts, F, P)
    check_listed(res, F, P, failed, 64)


def test_full_size(ctx):
    E, R, k = 4096, 33, 256
    pos, failed, F, P = C.case(E, R)
    res = hs.order_contrast(pos, failed, k=k, want_counts=True, ctx=ctx)
    check_listed(res, F, P, failed, k)
    for i in (0, 63, 64, 2047, 4095):
        assert np.array_equal(res.counts["n_fail_with"][i], F[i]) and np.array_equal(res.counts["n_pass_with"][i], P[i])
        assert np.array_equal(res.counts["n_fail_with"][:, i], F[:, i])
        assert np.array_equal(res.counts["n_pass_with"][:, i], P[:, i])
    rng = np.random.default_rng(4096)
    for b, a in rng.integers(0, E, (4096, 2)):
        if a == b:
            continue
        one, _, _ = hs.order_pair(pos, failed, int(b), int(a))
        c = res.counts[b, a]
        assert (int(c["n_fail_with"]), int(c["n_pass_with"])) == (int(one["n_fail_with"]), int(one["n_pass_with"]))
    hot = hs.order_contrast(pos, failed, k=k, ctx=ctx)
    check_listed(hot, F, P, failed, k)


def test_all_present_runs_are_antisymmetric(ctx):
    E, R = 129, 33
    rng = np.random.default_rng(129)
    pos = np.stack([rng.permutation(E) for _ in range(R)]).astype(np.uint32) * 7
    failed = (rng.random(R) < 0.4).astype(np.uint8)
    failed[0], failed[1] = 1, 0
    res = hs.order_contrast(pos, failed, k=256, want_counts=True, ctx=ctx)
    Fg = res.counts["n_fail_with"].astype(np.int64)
    Pg = res.counts["n_pass_with"].astype(np.int64)
    off = ~np.eye(E, dtype=bool)
    assert np.array_equal((Fg + Fg.T)[off], np.full(E * E - E, res.n_fail))
    assert np.array_equal((Pg + Pg.T)[off], np.full(E * E - E, res.n_pass))
    sc = Fg * res.n_pass - Pg * res.n_fail
    assert np.array_equal(sc, -sc.T)
    F, P = C.counts(pos, failed)
    check_counts(res.counts, F, P)
    check_listed(res, F, P, failed, 256)


def test_the_loop_from_a_storage_to_a_seed(ctx):
    """Labelled runs -> the discriminating pair -> a constraint -> seeds -> the best seed delivers the planted order."""
    E, R = 65, 33
    pos, failed, F, P = C.case(E, R)
    res = hs.order_contrast(pos, failed, k=64, ctx=ctx)
    assert (int(res.pairs[0]["before"]), int(res.pairs[0]["after"])) == (7, 3)
    cons = replay.constraints_from_pairs(res.pairs[:1], 1_000_000)
    assert cons == [(7, 3, 1_000_000)]
    n = 64
    hints = [f"hint-{i:03d}".encode() for i in range(n)]
    arrival = np.arange(n, dtype=np.int64) * 1_000_000
    policy = Replayable()
    policy.MaxInterval = 50_000_000
    r = policy.OrderSweep(hints, arrival, cons, seed_lo=0, n_seeds=4096, k=8, want_stats=False, ctx=ctx)
    best = replay.replayable_seeds(r.topk, range(4096))
    assert len(best) == 8 and int(r.topk[0]["n_fault"]) == 1
    policy.Seed = best[0]
    stats, slack = policy.order_slack(hints, arrival, cons)
    assert int(stats["n_satisfied"]) == 1 and slack[0] >= 0
    order, _, _ = policy.delivery_order(hints, arrival, np.arange(n, dtype=np.uint64))
    order = list(order)
    assert order.index(7) < order.index(3)


def test_naive_storage_labels_its_runs(ctx, golden, tmp_path):
    """Naive.OrderContrast on the ZooKeeper store: IsSuccessful labels the runs, a run without a readable result is
    skipped, and the rest equals order_contrast over run_positions."""
    traces = zk_store_traces(golden)
    write_store(str(tmp_path), traces)
    labels = {0: False, 1: True, 2: True, 3: True, 5: True}  # run 0 failed; run 4 has no result.json
    for i, ok in labels.items():
        with open(os.path.join(str(tmp_path), "%08x" % i, "result.json"), "w") as f:
            json.dump({"successful": ok, "required_time": 1}, f)
    st = hs.LoadStorage(str(tmp_path))
    runs = st.traces()
    sym = runs[0].symbols
    arr = np.arange(len(sym), dtype=np.int64)
    res = st.OrderContrast(sym, arr, k=64, want_counts=True, ctx=ctx)
    assert res.run_ids == [0, 1, 2, 3, 5]
    pos = hs.run_positions(sym, arr, [runs[i] for i in res.run_ids])
    failed = np.array([0 if labels[i] else 1 for i in res.run_ids], np.uint8)
    F, P = C.counts(pos, failed)
    check_counts(res.counts, F, P)
    check_listed(res, F, P, failed, 64)
    assert res.n_positive > 0


def test_two_calls_give_identical_bytes(ctx):
    pos, failed, _, _ = C.case(257, 65)
    a = hs.order_contrast(pos, failed, k=256, want_counts=True, ctx=ctx)
    b = hs.order_contrast(pos, failed, k=256, want_counts=True, ctx=ctx)
    assert a.pairs.tobytes() == b.pairs.tobytes() and a.counts.tobytes() == b.counts.tobytes()
    assert (a.n_fail, a.n_pass, a.n_positive) == (b.n_fail, b.n_pass, b.n_positive)
