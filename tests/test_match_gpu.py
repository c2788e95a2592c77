"""GPU: k_match_runs (nmz_match_runs, nmz_match_runs_dev, nmz_order_contrast_runs) against the numpy route
historystorage.run_positions / match_target on the grid of tests/match_cases.py, its stores reversed, many short
runs, a run of many tiles, a run that over-fills its one symbol, the device-pointer form on a non-default stream,
the contrast from the runs byte for byte, the ZooKeeper store, a matched row as a nearest-order target, and
run-to-run determinism."""
import ctypes
import json
import os

import numpy as np
import pytest

import contrast_ref as C
import match_cases as M
from namazu_amd import _lib, historystorage as hs
from namazu_amd.explorepolicy import Replayable
from test_visualize import write_store, zk_store_traces

pytestmark = pytest.mark.gpu
NONE = _lib.NMZ_NONE


@pytest.mark.parametrize("E,U", M.CASES)
def test_grid_stores_equal_run_positions(ctx, E, U):
    sym, arrival, runs, exp = M.case(E, U)
    got = hs.match_runs(sym, arrival, list(runs), ctx=ctx)
    assert got.dtype == np.uint32 and got.shape == exp.shape
    assert np.array_equal(got, exp)
    # the same store reversed: the long runs first, the empty run last
    back = hs.match_runs(sym, arrival, list(runs)[::-1], ctx=ctx)
    assert np.array_equal(back, exp[::-1])


def test_many_short_runs(ctx):
    """257 runs of lengths 0 .. 130 over 64 events: one-wave workgroups, several rounds of the grid stride."""
    sym, arrival, _, _ = M.case(64, 5)
    rng = np.random.default_rng(257)
    runs = [M.run(sym, int(L), rng) for L in rng.integers(0, 131, 257)]
    runs[0], runs[-1] = runs[0][:0], M.run(sym, 130, rng)
    exp = hs.run_positions(sym, arrival, runs)
    assert np.array_equal(hs.match_runs(sym, arrival, runs, ctx=ctx), exp)
    assert (exp != NONE).any() and (exp == NONE).any()


def test_one_run_of_many_tiles(ctx):
    """70,000 elements over (300, 40): 69 tiles of 1,024, the cursors carried from tile to tile."""
    sym, arrival, _, _ = M.case(300, 40)
    run = M.run(sym, 70_000, np.random.default_rng(70))
    # thin the early tiles so that events are still being matched late in the run
    keep = np.ones(len(run), bool)
    keep[:60_000] = np.random.default_rng(71).random(60_000) < 0.02
    run = np.where(keep, run, np.uint64(2))  # 2: even, not in the universe; positions stay
    exp = hs.run_positions(sym, arrival, [run])
    assert exp[exp != NONE].max() > 20_000
    assert np.array_equal(hs.match_runs(sym, arrival, [run], ctx=ctx), exp)


def test_one_symbol_over_full(ctx):
    """9,000 copies of the one symbol of (4096, 1): positions 0 .. 4,095 in (arrival, index) order, the rest
    dropped."""
    sym, arrival, _, _ = M.case(4096, 1)
    run = np.full(9000, sym[0], np.uint64)
    got = hs.match_runs(sym, arrival, [run], ctx=ctx)
    assert np.array_equal(got, hs.run_positions(sym, arrival, [run]))
    assert sorted(got[0].tolist()) == list(range(4096))
    assert np.array_equal(np.argsort(got[0]), np.lexsort((np.arange(4096), arrival)))


def _dev_match(plan, ts, E, stream, offset_rows=0):
    import torch
    d_off = torch.from_numpy(ts.off.view(np.int64)).cuda()
    d_sym = torch.from_numpy(ts.sym.view(np.int64)).cuda()
    d_pos = torch.zeros((len(ts) + offset_rows) * E, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()  # the copies and the zeroing ran on torch's current stream
    out = d_pos[offset_rows * E:]
    plan.runs_dev(d_off.data_ptr(), d_sym.data_ptr(), len(ts), out.data_ptr(), stream.cuda_stream)
    stream.synchronize()
    return out.cpu().numpy().view(np.uint32).reshape(len(ts), E)


@pytest.mark.parametrize("E,U", [(65, 65), (1024, 300), (4096, 300)])
def test_dev_form_on_a_side_stream(ctx, E, U):
    import torch
    sym, arrival, runs, exp = M.case(E, U)
    side = torch.cuda.Stream()
    plan = hs.MatchPlan(sym, arrival, ctx=ctx)
    try:
        assert (plan.n_events, plan.n_symbols) == (E, U)
        ts = hs.TraceSet(list(runs))
        got = _dev_match(plan, ts, E, side)
        assert np.array_equal(got, exp)
        assert np.array_equal(got, hs.match_runs(sym, arrival, list(runs), ctx=ctx))
        # rows that start one row into a buffer: with E = 65 the rows are not 16-byte aligned
        assert np.array_equal(_dev_match(plan, ts, E, side, offset_rows=1), exp)
        # no runs: nothing is enqueued
        plan.runs_dev(0, 0, 0, 0, side.cuda_stream)
    finally:
        plan.close()


def _labels(pos):
    """Labels as contrast_ref makes them: a run fails iff it holds events 7 % E and 3 % E in that order, flipped
    for every tenth run; at least one run of each label."""
    E = pos.shape[1]
    failed = ((pos[:, 7 % E] < pos[:, 3 % E]) ^ (np.arange(len(pos)) % 10 == 9)).astype(np.uint8)
    if not failed.any():
        failed[0] = 1
    if failed.all():
        failed[-1] = 0
    return failed


@pytest.mark.parametrize("E,U,R", [(65, 65, 33), (1024, 300, 257)])
def test_order_contrast_runs_byte_identical(ctx, E, U, R):
    sym, arrival, _, _ = M.case(E, U)
    rng = np.random.default_rng(R)
    runs = [M.run(sym, int(L), rng) for L in rng.integers(E // 2, 2 * E, R)]
    pos = hs.run_positions(sym, arrival, runs)
    failed = _labels(pos)
    for k, want in ((64, True), (256, False), (0, False)):
        exp = hs.order_contrast(pos, failed, k=k, want_counts=want, ctx=ctx)
        got = hs.order_contrast_runs(sym, arrival, runs, failed, k=k, want_counts=want, ctx=ctx)
        assert got.pairs.tobytes() == exp.pairs.tobytes()
        assert (got.n_fail, got.n_pass, got.n_positive) == (exp.n_fail, exp.n_pass, exp.n_positive)
        if want:
            assert got.counts.tobytes() == exp.counts.tobytes()
        else:
            assert got.counts is None
    assert exp.n_fail > 0 and exp.n_pass > 0
    # and through nmz_match_runs' rows
    mid = hs.order_contrast(hs.match_runs(sym, arrival, runs, ctx=ctx), failed, k=64, ctx=ctx)
    ref = hs.order_contrast(pos, failed, k=64, ctx=ctx)
    assert mid.pairs.tobytes() == ref.pairs.tobytes() and ref.n_positive > 0


def test_naive_storage_contrast_equals_the_run_positions_route(ctx, golden, tmp_path):
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
    used = [runs[i] for i in res.run_ids]
    pos = hs.run_positions(sym, arr, used)
    assert np.array_equal(hs.match_runs(sym, arr, used, ctx=ctx), pos)
    failed = np.array([0 if labels[i] else 1 for i in res.run_ids], np.uint8)
    exp = hs.order_contrast(pos, failed, k=64, want_counts=True, ctx=ctx)
    assert res.pairs.tobytes() == exp.pairs.tobytes() and res.counts.tobytes() == exp.counts.tobytes()
    assert (res.n_fail, res.n_pass, res.n_positive) == (exp.n_fail, exp.n_pass, exp.n_positive)
    assert res.n_positive > 0


def test_a_matched_row_is_a_nearest_order_target(ctx):
    sym, arrival, runs, exp = M.case(300, 40)
    r = M.LENGTHS.index(1023)
    row = hs.match_runs(sym, arrival, [runs[r]], ctx=ctx)[0]
    ref = hs.match_target(sym, arrival, runs[r])
    assert np.array_equal(row, ref) and (row != NONE).sum() > 100
    p = Replayable()
    p.MaxInterval = 10**8
    hints = [f"hint-{i}" for i in range(300)]
    a = p.NearestOrders(hints, arrival, target_pos=row, seed_lo=0, n_seeds=64, ctx=ctx)
    b = p.NearestOrders(hints, arrival, target_pos=ref, seed_lo=0, n_seeds=64, ctx=ctx)
    assert a.stats.tobytes() == b.stats.tobytes() and (a.n_counted, a.n_pairs) == (b.n_counted, b.n_pairs)
    assert a.n_counted == int((row != NONE).sum())


def test_two_calls_give_identical_bytes(ctx):
    sym, arrival, runs, _ = M.case(4096, 300)
    a = hs.match_runs(sym, arrival, list(runs), ctx=ctx)
    b = hs.match_runs(sym, arrival, list(runs), ctx=ctx)
    assert a.tobytes() == b.tobytes()
    failed = np.arange(len(runs), dtype=np.uint8) % 2
    x = hs.order_contrast_runs(sym, arrival, list(runs), failed, k=64, ctx=ctx)
    y = hs.order_contrast_runs(sym, arrival, list(runs), failed, k=64, ctx=ctx)
    assert x.pairs.tobytes() == y.pairs.tobytes() and x.n_positive == y.n_positive
