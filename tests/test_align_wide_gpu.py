"""GPU: k_ed_align_wide (nmz_ed_align_wide_pairs, nmz_ed_align_wide_pairs_dev, Naive.DiffSimilar beyond band 64)
against the host form nmz_ed_align_wide_host, which tests/test_align_wide_host.py ties to the definition.

Every slot of every pair is compared: the distance, the ops in forward order and the sentinels behind them. The
shapes are the smallest at which this kernel can still go wrong: lengths around the 64-row blocks at the bands where
the cells per thread change, the band's two edge cells, more pairs than the plan has slots, one pair whose history
spans a thousand row blocks, the device-pointer form on a side stream, and narrow bands through the wide entry
points."""
import ctypes
import functools

import numpy as np
import pytest

import align_ref as AR
import ed_cases as EC
from namazu_amd import _lib
from namazu_amd import historystorage as hs
from test_align_wide_host import constructed, wide_slots

pytestmark = pytest.mark.gpu

NONE3 = (_lib.NMZ_NONE,) * 3


def expected(trs, pairs, w, memo=None):
    """dist[P], ops[P][w] of nmz_ed_align_wide_host, computed once per distinct pair."""
    dist = np.zeros(len(pairs), np.uint32)
    ops = np.zeros((len(pairs), w), _lib.EDIT_OP_DTYPE)
    memo = {} if memo is None else memo
    for p, (i, j) in enumerate(np.asarray(pairs).tolist()):
        if (i, j) not in memo:
            memo[(i, j)] = wide_slots(trs[i], trs[j], w)
        dist[p], ops[p] = memo[(i, j)]
    return dist, ops


def check(es, dist, ops):
    assert np.array_equal(es.dist, dist), np.nonzero(es.dist != dist)[0][:10]
    assert es.ops.shape == ops.shape
    bad = np.nonzero((es.ops != ops).any(axis=1))[0] if ops.shape[1] else []
    assert len(bad) == 0, (bad[:10], es.dist[bad[0]], es.ops[bad[0]][:8], ops[bad[0]][:8])


def _runs(t, n_del, n_ins, rng):
    """t with n_del elements deleted and n_ins inserted, each in runs of up to 40."""
    t = list(t)
    for total, ins in ((n_del, False), (n_ins, True)):
        left = total
        while left:
            k = min(left, int(rng.integers(8, 41)))
            p = int(rng.integers(0, len(t) - (0 if ins else k) + 1))
            t[p:p + (0 if ins else k)] = [int(x) for x in rng.integers(0, 4, size=k)] if ins else []
            left -= k
    return np.array(t, np.int64)


@functools.lru_cache(maxsize=None)
def family():
    """42 traces over {0, 1, 2, 3}. Every length L of the row-block joints comes plain (a prefix of one base, so two
    plain traces are exactly their length difference apart, up to 300), lightly edited (3 point edits; from L = 255
    also a run of 70 inserted, so the path leaves the diagonal by more than 64) and heavily edited (from L = 127:
    65 elements deleted in runs, which is exactly 65 edits from the plain one -- the first wide distance; below:
    12 point edits). Six long traces put pairs beyond every band: two of 1,400 and 1,500 elements over disjoint
    halves of the alphabet (Lev = 1,500: the cut-off decides, at every band), one 80 run edits from the first, and
    three of 650 to 700 elements."""
    rng = np.random.default_rng(2025)
    base = rng.integers(0, 4, size=300).astype(np.int64)
    out = []
    for L in (0, 1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 300):
        light = EC._edited(base[:L], 3, 4, rng)
        out += [base[:L].copy(), _runs(light, 0, 70, rng) if L >= 255 else light,
                _runs(base[:L], 65, 0, rng) if L >= 127 else EC._edited(base[:L], 12, 4, rng)]
    l1 = rng.integers(0, 2, size=1400).astype(np.int64)
    l4 = rng.integers(0, 4, size=700).astype(np.int64)
    out += [l1, rng.integers(2, 4, size=1500).astype(np.int64), _runs(l1, 40, 40, rng), l4, _runs(l4, 100, 50, rng),
            rng.integers(2, 4, size=650).astype(np.int64)]
    return tuple(EC.encode(t) for t in out)


# ---- 1. the instantiation joints -------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", [65, 127, 128, 255, 256, 383, 384, 639, 640, 1024])
def test_instantiation_joints(ctx, w):
    """The kernel has C = 1, 2, 3, 5, 9 cells per thread for w <= 127, 255, 383, 639, 1,024: every band at which C
    changes, its neighbour below, the first wide band and the last. All ordered pairs of the family."""
    trs = family()
    pairs = EC.all_ordered_pairs(len(trs))
    dist, ops = expected(trs, pairs, w)
    print(w, "within", int((dist <= w).sum()), "beyond", int((dist > w).sum()), "within and > 64",
          int(((dist > 64) & (dist <= w)).sum()))
    assert (dist <= w).sum() >= 16 and (dist > w).sum() >= 16
    if w <= 256:
        assert ((dist > 64) & (dist <= w)).sum() >= 8
    check(hs.edit_scripts_wide(hs.TraceSet(list(trs)), pairs, w, ctx=ctx), dist, ops)


# ---- 2. the band's edges ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", [65, 128, 1024])
def test_edges(ctx, w):
    """The constructed rows of tests/test_align_wide_host.py on the device, in both pair orders: a script that fills
    every slot on the band's edge cell d = 2 w, the other edge d = 0, the cut-off at equal lengths, and the
    rotation at dist = band and dist = band + 1."""
    for a, b, band, dist, sc in constructed(w):
        trs = [EC.encode(a), EC.encode(b)]
        pairs = np.array([[0, 1], [1, 0], [0, 0]], np.uint32)
        want_d, want_o = expected(trs, pairs, band)
        assert want_d[0] == dist and want_d[2] == 0
        es = hs.edit_scripts_wide(hs.TraceSet(trs), pairs, band, ctx=ctx)
        check(es, want_d, want_o)
        if sc is None:
            assert es.script(0) is None
        else:
            assert AR.as_tuples(es.script(0)) == sc and AR.as_tuples(es.ops[0, dist:]) == [NONE3] * (band - dist)


# ---- 3. narrow bands through the wide entry points ---------------------------------------------------------------------
@pytest.mark.parametrize("w", [0, 8, 64])
def test_narrow_bands_equal_the_narrow_entry_points(ctx, w):
    trs = family()[:36:2] + family()[36:38]
    pairs = EC.all_ordered_pairs(len(trs))
    ts = hs.TraceSet(list(trs))
    narrow = hs.edit_scripts(ts, pairs, w, ctx=ctx)
    es = hs.edit_scripts_wide(ts, pairs, w, ctx=ctx)
    assert es.ops.shape == (len(pairs), w) and es.ops.dtype == narrow.ops.dtype
    assert es.dist.tobytes() == narrow.dist.tobytes() and es.ops.tobytes() == narrow.ops.tobytes()
    assert (es.dist <= w).sum() >= 16 and (es.dist > w).sum() >= 16
    plan, nplan = hs.AlignWidePlan(w, 300, ctx=ctx), hs.AlignPlan(w, 300, ctx=ctx)
    try:
        assert (plan.slots, plan.history_bytes) == (nplan.slots, nplan.history_bytes)
    finally:
        plan.close()
        nplan.close()


# ---- 4. more pairs than slots ----------------------------------------------------------------------------------------
def test_slot_reuse(ctx):
    """2 * slots + 3 pairs at w = 65 over traces of 0 .. 140 elements, long and short mixed, with (i, i) pairs and
    duplicates: a slot's stale history is longer than the next pair's."""
    w = 65
    rng = np.random.default_rng(65)
    base = rng.integers(0, 4, size=140).astype(np.int64)
    trs = []
    for L in (0, 1, 5, 30, 64, 65, 70, 128, 129, 140):
        trs += [base[:L].copy(), EC._edited(base[:L], 4, 4, rng), EC._edited(base[:L], 30, 4, rng)]
    trs = [EC.encode(t[:140]) for t in trs]
    plan = hs.AlignWidePlan(w, 140, ctx=ctx)
    try:
        slots = plan.slots
        assert slots >= 1 and plan.history_bytes >= slots * 3 * 64 * 64  # 3 row blocks of 64 rows of 64 bytes
    finally:
        plan.close()
    n = 2 * slots + 3
    pairs = rng.integers(0, len(trs), size=(n, 2)).astype(np.uint32)
    pairs[::97, 1] = pairs[::97, 0]  # (i, i)
    pairs[1::2] = pairs[0:2 * (n // 2):2][rng.permutation(n // 2)]  # duplicates
    dist, ops = expected(trs, pairs, w)
    assert (dist == 0).sum() >= 8 and ((dist > 0) & (dist <= w)).sum() >= 100 and (dist > w).sum() >= 100
    check(hs.edit_scripts_wide(hs.TraceSet(trs), pairs, w, ctx=ctx), dist, ops)


# ---- 5. a long history -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_edits,in_band", [(100, True), (140, False)])
def test_long_pair(ctx, n_edits, in_band):
    from test_align_gpu import _long_pair
    a, b = _long_pair(n_edits)
    w = 128
    pairs = np.array([[0, 1], [1, 0]], np.uint32)
    dist, ops = expected([a, b], pairs, w)
    assert (dist[0] == n_edits) if in_band else (dist[0] == w + 1)
    es = hs.edit_scripts_wide(hs.TraceSet([a, b]), pairs, w, ctx=ctx)
    check(es, dist, ops)
    if in_band:
        sc = AR.as_tuples(es.script(0))
        assert AR.replay(a, b, sc) and sc[0][0] < 70000 // 8 and sc[-1][0] > 70000 * 7 // 8  # across the history
    else:
        assert es.script(0) is None and es.script(1) is None


# ---- 6. the device-pointer form --------------------------------------------------------------------------------------
def test_dev_form_on_a_side_stream(ctx):
    import torch
    w = 100
    trs = list(family()[:36])
    n = len(trs)
    long_one = EC.encode(np.arange(400))  # longer than the plan's max_len
    ts = hs.TraceSet(trs + [long_one])
    pairs = EC.all_ordered_pairs(n)[::3]
    pairs = np.concatenate([pairs[:100], [[n, 0], [0, n], [n, n]], pairs[100:]]).astype(np.uint32)
    is_long = (pairs == n).any(axis=1)
    dist, ops = expected(trs + [long_one], np.where(pairs == n, 0, pairs), w)
    dist[is_long] = _lib.NMZ_NONE
    ops[is_long] = NONE3
    assert ((dist > 64) & (dist <= w)).sum() >= 8 and ((dist > w) & ~is_long).sum() >= 16
    plan = hs.AlignWidePlan(w, max(len(t) for t in trs), ctx=ctx)
    try:
        side = torch.cuda.Stream()
        d_off = torch.from_numpy(ts.off.view(np.int64)).cuda()
        d_sym = torch.from_numpy(ts.sym.view(np.int64)).cuda()
        d_pairs = torch.from_numpy(pairs.view(np.int32)).cuda()
        for _ in range(2):  # the same plan again: the slots hold the last launch's history
            d_dist = torch.full((len(pairs),), 7, dtype=torch.int32, device="cuda")
            d_ops = torch.full((len(pairs) * w * 3,), 7, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()  # the copies and the fills ran on torch's current stream
            plan.pairs_dev(d_off.data_ptr(), d_sym.data_ptr(), d_pairs.data_ptr(), len(pairs), d_dist.data_ptr(),
                           d_ops.data_ptr(), side.cuda_stream)
            side.synchronize()
            got_d = d_dist.cpu().numpy().view(np.uint32)
            got_o = d_ops.cpu().numpy().view(np.uint32).reshape(len(pairs), w, 3)
            assert np.array_equal(got_d, dist)
            want_o = np.stack([ops["a_pos"], ops["b_pos"], ops["kind"]], axis=2)
            assert np.array_equal(got_o, want_o)
        plan.pairs_dev(0, 0, 0, 0, 0, 0, side.cuda_stream)  # no pairs: nothing is enqueued
    finally:
        plan.close()
    short = ~is_long
    assert np.array_equal(hs.ed_pairs(ts, pairs[short], w, ctx=ctx), dist[short])


# ---- 7. Naive.DiffSimilar beyond band 64 -----------------------------------------------------------------------------
def test_diff_similar_at_band_200(golden, tmp_path):
    """The zk store plus two runs made far from run 0: the other stored runs' actions in front of run 0's (103
    elements more) and two of them behind it (67 more)."""
    from test_visualize import write_store, zk_store_traces
    tr = zk_store_traces(golden)
    (a0, e0), (a1, e1), (a2, e2), (a3, e3) = tr[:4]
    tr.append((a1 + a2 + a3 + a0, e1 + e2 + e3 + e0))
    tr.append((a0 + a1 + a2, e0 + e1 + e2))
    write_store(str(tmp_path), tr)
    st = hs.LoadStorage(str(tmp_path))
    runs = st.traces()
    band = 200
    got = st.DiffSimilar(runs[0], k=8, band=band)
    assert [i for i, _, _ in got][:3] == [0, 4, 5] and len(got) == 8
    by_id = {i: (d, sc) for i, d, sc in got}
    for i, (d, sc) in by_id.items():
        assert len(sc) == d
        assert AR.replay(runs[i].symbols, runs[0].symbols, AR.as_tuples(sc))
        assert wide_slots(runs[i].symbols, runs[0].symbols, band)[0] == d
    assert 64 < by_id[7][0] <= 67 and 64 < by_id[6][0] <= 103  # the neighbours beyond 64 are there
    assert by_id[4][0] == 0 and len(by_id[4][1]) == 0
