"""GPU: k_ed_align (nmz_ed_align_pairs, nmz_ed_align_pairs_dev, Naive.DiffSimilar) against the host form
nmz_ed_align_host, which tests/test_align_host.py ties to the definition op for op.

Every slot of every pair is compared: the distance, the ops in forward order and the sentinels behind them. The
shapes: the structured families of tests/ed_cases.py in both roles, lengths around the 64-row blocks at the bands
where the cells per lane change (w = 31 | 32, 63 | 64), more pairs than the plan has slots, one pair whose history
spans a thousand staged blocks, and the device-pointer form on a side stream."""
import ctypes
import functools

import numpy as np
import pytest

import align_ref as AR
import ed_cases as EC
from namazu_amd import _lib
from namazu_amd import historystorage as hs

pytestmark = pytest.mark.gpu

BV = ["bv-w5", "bv-w8", "bv-w16", "bv-w32", "bv-w33", "bv-w50", "bv-w64", "bv-per8", "bv-per32", "bv-per64"]


def host_slots(a, b, w):
    """(dist, ops[w]) of nmz_ed_align_host: all `band` slots, sentinels included."""
    a, b = np.ascontiguousarray(a, np.uint64), np.ascontiguousarray(b, np.uint64)
    dist = ctypes.c_uint32()
    ops = np.zeros(w, _lib.EDIT_OP_DTYPE)
    _lib.check(_lib.load().nmz_ed_align_host(_lib.ptr(a), len(a), _lib.ptr(b), len(b), w, ctypes.byref(dist),
                                             _lib.ptr(ops) if w else None))
    return dist.value, ops


def expected(trs, pairs, w):
    dist = np.zeros(len(pairs), np.uint32)
    ops = np.zeros((len(pairs), w), _lib.EDIT_OP_DTYPE)
    memo = {}
    for p, (i, j) in enumerate(np.asarray(pairs).tolist()):
        if (i, j) not in memo:
            memo[(i, j)] = host_slots(trs[i], trs[j], w)
        dist[p], ops[p] = memo[(i, j)]
    return dist, ops


def check(es, dist, ops):
    assert np.array_equal(es.dist, dist), np.nonzero(es.dist != dist)[0][:10]
    assert es.ops.shape == ops.shape
    bad = np.nonzero((es.ops != ops).any(axis=1))[0] if ops.shape[1] else []
    assert len(bad) == 0, (bad[:10], es.ops[bad[0]][:8], ops[bad[0]][:8])


# ---- 1. the families, both roles -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", BV)
def test_families(ctx, name):
    trs, w = EC.traces(name), EC.band(name)
    pairs = EC.all_ordered_pairs(len(trs))
    dist, ops = expected(trs, pairs, w)
    assert np.array_equal(dist.reshape(len(trs), -1), EC.reference(name))
    es = hs.edit_scripts(hs.TraceSet(list(trs)), pairs, w, ctx=ctx)
    check(es, dist, ops)
    p = int(np.argmax(np.where(dist <= w, dist, 0)))
    assert len(es.script(p)) == dist[p] and AR.replay(trs[pairs[p][0]], trs[pairs[p][1]], AR.as_tuples(es.script(p)))
    far = np.nonzero(dist > w)[0]
    if len(far):
        assert es.script(int(far[0])) is None


# ---- 2. short lengths: the cells-per-lane and block joints -----------------------------------------------------------
@functools.lru_cache(maxsize=None)
def short_traces():
    rng = np.random.default_rng(2024)
    base = rng.integers(0, 4, size=130).astype(np.int64)
    out = []
    for L in (0, 1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 130):
        out += [base[:L].copy(), EC._edited(base[:L], 2, 4, rng), EC._edited(base[:L], 6, 4, rng)]
    return tuple(EC.encode(t) for t in out)


@pytest.mark.parametrize("w", [1, 8, 31, 32, 63, 64])
def test_short_lengths(ctx, w):
    trs = short_traces()
    pairs = EC.all_ordered_pairs(len(trs))
    dist, ops = expected(trs, pairs, w)
    assert (dist <= w).sum() >= 36 and (dist > w).sum() >= 36
    check(hs.edit_scripts(hs.TraceSet(list(trs)), pairs, w, ctx=ctx), dist, ops)


def test_band_zero(ctx):
    trs = short_traces()
    pairs = EC.all_ordered_pairs(len(trs))
    es = hs.edit_scripts(hs.TraceSet(list(trs)), pairs, 0, ctx=ctx)
    want = np.array([0 if np.array_equal(trs[i], trs[j]) else 1 for i, j in pairs.tolist()], np.uint32)
    assert np.array_equal(es.dist, want) and es.ops.shape == (len(pairs), 0)


# ---- 3. more pairs than slots ----------------------------------------------------------------------------------------
def test_slot_reuse(ctx):
    trs, w = EC.traces("bv-w8"), 8
    rng = np.random.default_rng(8)
    pairs = rng.integers(0, len(trs), size=(20000, 2)).astype(np.uint32)
    pairs[::97, 1] = pairs[::97, 0]  # (i, i)
    pairs[1::2] = pairs[0:-1:2][rng.permutation(10000)]  # duplicates
    plan = hs.AlignPlan(w, max(len(t) for t in trs), ctx=ctx)
    try:
        assert 1 <= plan.slots < len(pairs) and plan.history_bytes >= plan.slots * 2 * 8 * 64
    finally:
        plan.close()
    dist, ops = expected(trs, pairs, w)
    check(hs.edit_scripts(hs.TraceSet(list(trs)), pairs, w, ctx=ctx), dist, ops)


# ---- 4. a long pair --------------------------------------------------------------------------------------------------
def _long_pair(n_edits):
    rng = np.random.default_rng(70000)
    a = rng.integers(0, 1000, size=70000).astype(np.int64)
    b = a.tolist()
    at = np.sort(rng.choice(np.arange(100, 69900, 50), n_edits, replace=False))[::-1]
    for t, p in enumerate(at.tolist()):  # back to front, so the positions stay those of a
        if t % 3 == 0:
            b[p] = 1000 + t
        elif t % 3 == 1:
            del b[p]
        else:
            b.insert(p, 2000 + t)
    return EC.encode(a), EC.encode(np.array(b, np.int64))


@pytest.mark.parametrize("n_edits,in_band", [(40, True), (70, False)])
def test_long_pair(ctx, n_edits, in_band):
    a, b = _long_pair(n_edits)
    w = 64
    pairs = np.array([[0, 1], [1, 0]], np.uint32)
    dist, ops = expected([a, b], pairs, w)
    assert (dist[0] == n_edits) if in_band else (dist[0] == w + 1)
    es = hs.edit_scripts(hs.TraceSet([a, b]), pairs, w, ctx=ctx)
    check(es, dist, ops)
    if in_band:
        sc = AR.as_tuples(es.script(0))
        assert AR.replay(a, b, sc) and sc[0][0] < 70000 // 8 and sc[-1][0] > 70000 * 7 // 8  # across the history
    else:
        assert es.script(0) is None and es.script(1) is None


# ---- 5. the device-pointer form --------------------------------------------------------------------------------------
def test_dev_form_on_a_side_stream(ctx):
    import torch
    name, w = "bv-w33", 33
    trs = list(EC.traces(name))
    n = len(trs)
    long_one = EC.encode(np.arange(400))  # longer than the plan's max_len
    ts = hs.TraceSet(trs + [long_one])
    pairs = EC.all_ordered_pairs(n)
    pairs = np.concatenate([pairs[:100], [[n, 0], [0, n], [n, n]], pairs[100:]]).astype(np.uint32)
    is_long = (pairs == n).any(axis=1)
    dist, ops = expected(trs + [long_one], np.where(pairs == n, 0, pairs), w)
    dist[is_long] = _lib.NMZ_NONE
    ops[is_long] = (_lib.NMZ_NONE,) * 3
    plan = hs.AlignPlan(w, max(len(t) for t in trs), ctx=ctx)
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


# ---- 6. Naive.DiffSimilar --------------------------------------------------------------------------------------------
def test_diff_similar_on_the_zk_store(golden, tmp_path):
    from test_visualize import write_store, zk_store_traces
    write_store(str(tmp_path), zk_store_traces(golden))
    st = hs.LoadStorage(str(tmp_path))
    runs = st.traces()
    band = 32
    got = st.DiffSimilar(runs[0], k=6, band=band)
    ids = [i for i, _, _ in got]
    assert ids[:3] == [0, 4, 5] and len(got) == len([1 for i, d in st.SearchSimilar(runs[0], 6, band) if d <= band])
    for i, d, sc in got:
        assert len(sc) == d
        assert AR.replay(runs[i].symbols, runs[0].symbols, AR.as_tuples(sc))
        assert host_slots(runs[i].symbols, runs[0].symbols, band)[0] == d
    by_id = {i: (d, sc) for i, d, sc in got}
    assert runs[0].Equals(runs[4]) and by_id[4][0] == 0 and len(by_id[4][1]) == 0
    assert any(d > 0 for _, d, _ in got) or len(got) == 3
