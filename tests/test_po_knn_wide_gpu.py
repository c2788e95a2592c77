"""GPU: the PO k-NN search over bands 65 .. 1,024 (k_po_knn_wide; the nmz_po_knn_wide* entry points;
PoSimilarityIndex(wide=True), po_knn_wide, Naive.SearchSimilarPOWide and the po_search keyword of DiffSimilar /
DiffFailing above band 64) against the host forms: nmz_ed_align_po_host for the distances, tests/po_knn_ref.py for
the lists, and the nine counters that tests/po_knn_wide_cases.py makes from the host forms.

Every id and distance of every list is compared, and all nine counters. The bands are the two sides of every joint of
the cells per thread (127 / 128, 255 / 256, 383 / 384, 639 / 640), the first wide band 65 and the last 1,024; the
"cut" family (28 traces, five entities) puts hundreds of pairs per band through the filters and then beyond the band
inside the DP, dozens onto the per-entity length check, and at band 1,024 entity steps onto every cell count; the
42-trace family adds projections of 0, 1, 63, 64 and 65 elements on the staging joints, 38 entities and the length-sum
counter."""
import json
import os

import numpy as np
import pytest

import po_knn_ref as KR
import po_knn_wide_cases as WC
from namazu_amd import _lib
from namazu_amd import historystorage as hs
from test_align_po_host import gpu_family, interleavings, po_slots

pytestmark = pytest.mark.gpu

NONE = _lib.NMZ_NONE
NO_FILTER, WHOLE_BLOCKS, FULL_BAND = (_lib.NMZ_PO_KNN_OPT_NO_FILTER, _lib.NMZ_PO_KNN_OPT_WHOLE_BLOCKS,
                                      _lib.NMZ_PO_KNN_OPT_FULL_BAND)


def same_lists(got, want, what):
    assert np.array_equal(got[0], want[0]), what
    assert np.array_equal(got[1], want[1]), what


def wide_index(key, w, ctx, opts=0, wide=True):
    ts, ent, G = WC.store(key)
    return hs.PoSimilarityIndex(ts, ent, w, ctx=ctx, n_entities=G, max_queries=64, max_query_elems=int(ts.off[-1]),
                                opts=opts, wide=wide)


# ---- 1. the joint bands against the host -----------------------------------------------------------------------------
@pytest.mark.parametrize("key,bands", [("cut", WC.BANDS), ("mod2", WC.BANDS), ("sparse", (65, 128, 256, 1024))])
def test_joint_bands(ctx, key, bands):
    """Store = queries = the family. k = 64 past the store's size checks the NMZ_NONE tail; q_self = NULL lets each
    trace find itself at 0 first."""
    ts, ent, G = WC.store(key)
    n = len(ts)
    D = WC.matrices(key)[0]
    beyond = mid = 0
    for w in bands:
        Dw = np.minimum(D, w + 1)
        index = wide_index(key, w, ctx)
        try:
            for k in (1, 64):
                for q_self in (np.arange(n, dtype=np.uint32), None):
                    got = index.query_csr(ts, ent, k, q_self)
                    same_lists(got, KR.knn(Dw, k, q_self), (key, w, k, q_self is None))
                    c = index.counters()
                    print(key, w, k, q_self is None, c)
                    assert c == WC.expected_counters(key, w, self_excluded=q_self is not None), (key, w, k)
                    if k == 64:
                        assert (got[0][:, n - (q_self is not None):] == NONE).all()
            beyond += c["dp"] - c["in_band"]
            mid += int(((D > 64) & (D <= w)).sum())
            bytes_, blocks, waves = index.info()
            assert bytes_ > 0 and blocks >= 1 and waves == 4 * blocks  # four waves per workgroup
        finally:
            index.close()
    assert mid >= 16 and (key == "sparse" or beyond >= 16)
    # the one-shot entry point: the same lists
    w = bands[2]
    q_self = np.arange(n, dtype=np.uint32)
    same_lists(hs.po_knn_wide(ts, ent, ts, ent, 8, w, n_entities=G, q_self=q_self, ctx=ctx),
               KR.knn(np.minimum(D, w + 1), 8, q_self), (key, "one shot"))


# ---- 2. the options ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", ["cut", "mod2"])
def test_options_at_band_256(ctx, key):
    """NO_FILTER, WHOLE_BLOCKS, FULL_BAND and their combinations: the default's bytes; the counters as computed, with
    FULL_BAND every step on the counter of CMAX = 3."""
    w = 256
    ts, ent, G = WC.store(key)
    n = len(ts)
    q_self = np.arange(n, dtype=np.uint32)
    lists, steps = {}, {}
    for opts in range(8):
        index = wide_index(key, w, ctx, opts=opts)
        try:
            lists[opts] = index.query_csr(ts, ent, 64, q_self)
            c = index.counters()
            assert c == WC.expected_counters(key, w, no_filter=bool(opts & NO_FILTER), full_band=bool(opts & FULL_BAND))
            steps[opts] = [c[name] for name in index.STEP_NAMES]
            if opts & WHOLE_BLOCKS:
                assert index.info()[1] == n  # one item per (query, block)
            else:
                assert index.info()[1] > n
        finally:
            index.close()
    same_lists(lists[0], KR.knn(np.minimum(WC.matrices(key)[0], w + 1), 64, q_self), key)
    for opts in range(1, 8):
        assert lists[0][0].tobytes() == lists[opts][0].tobytes() and lists[0][1].tobytes() == lists[opts][1].tobytes()
    assert steps[0][0] > 0 and steps[0][1] > 0 and steps[0][2] > 0  # the default spreads over C = 1, 2, 3
    assert steps[FULL_BAND] == [0, 0, sum(steps[0]), 0, 0]
    assert sum(steps[NO_FILTER]) >= sum(steps[0])


# ---- 3. bands 0, 8 and 64 through the wide entry points ---------------------------------------------------------------
@pytest.mark.parametrize("w", [0, 8, 64])
def test_narrow_bands_through_the_wide_entry_points(ctx, w):
    """A band <= 64 runs the narrow kernel: the narrow entry points' bytes and four counters, no entity step."""
    key = "mod2"
    ts, ent, G = WC.store(key)
    q_self = np.arange(len(ts), dtype=np.uint32)
    narrow, wide = wide_index(key, w, ctx, wide=False), wide_index(key, w, ctx, opts=FULL_BAND)
    try:
        for k, qs in ((8, q_self), (64, None)):
            a, b = narrow.query_csr(ts, ent, k, qs), wide.query_csr(ts, ent, k, qs)
            assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
            cn, cw = narrow.counters(), wide.counters()
            assert len(cn) == 4 and len(cw) == 9 and all(cw[name] == v for name, v in cn.items())
            assert all(cw[name] == 0 for name in wide.STEP_NAMES)
            assert narrow.info() == wide.info()
        assert (b[1] <= w).sum() >= 42
    finally:
        narrow.close()
        wide.close()
    a = hs.po_knn(ts, ent, ts, ent, 8, w, n_entities=G, q_self=q_self, ctx=ctx)
    b = hs.po_knn_wide(ts, ent, ts, ent, 8, w, n_entities=G, q_self=q_self, ctx=ctx)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


# ---- 4. one entity -----------------------------------------------------------------------------------------------------
def test_one_entity_equals_the_exact_wide_search(ctx):
    """n_entities = 1 at band 128: nmz_ed_plan_query_knn's lists (SimilarityIndex.query) and the host's."""
    w = 128
    trs = gpu_family("mod2")[0]
    ts = hs.TraceSet(list(trs))
    n = len(ts)
    ent = np.zeros(int(ts.off[-1]), np.uint32)
    D = np.array([[po_slots(trs[i], ent[:len(trs[i])], trs[j], ent[:len(trs[j])], 1, w)[0] for j in range(n)]
                  for i in range(n)], np.uint32)
    assert ((D > 64) & (D <= w)).sum() >= 16 and (D > w).sum() >= 16
    index = hs.PoSimilarityIndex(ts, ent, w, ctx=ctx, n_entities=1, max_queries=64, max_query_elems=int(ts.off[-1]),
                                 wide=True)
    exact = hs.SimilarityIndex(ts, w, ctx=ctx)
    try:
        for k in (8, 64):
            got = index.query_csr(ts, ent, k)
            same_lists(got, KR.knn(D, k), (w, k))
            same_lists(got, exact.query(list(trs), k), (w, k, "SimilarityIndex"))
    finally:
        index.close()
        exact.close()


# ---- 5. candidate-block joints and ties --------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 63, 64, 65, 129])
def test_candidate_blocks_and_ties(ctx, N):
    """Interleavings of three entities' fixed sequences at band 65: dozens of candidates tie at 0 and at 1 .. 4, so
    the id order decides."""
    w, k = 65, 64
    trs = interleavings(np.random.default_rng(2000 + N), N - 8 if N > 8 else N, 8 if N > 8 else 0,
                        lens=(40, 64, 70))
    singles = [hs.SingleTrace(s, entities=["e%d" % g for g in e]) for s, e in trs]
    ts, ent, names = hs.po_entities(singles)
    assert len(names) == 3
    members = sorted({0, N // 3, N // 2, N - 1})
    D = np.array([[po_slots(trs[m][0], trs[m][1], s, e, 3, w)[0] for s, e in trs] for m in members], np.uint32)
    if N > 8:
        assert (D == 0).sum() >= N - 8 and ((D >= 1) & (D <= w)).sum() >= 8
    index = hs.PoSimilarityIndex(ts, ent, w, names, ctx=ctx, wide=True)
    try:
        queries = [singles[m] for m in members]
        for q_self in (np.array(members, np.uint32), None):
            got = index.query(queries, k, q_self)
            same_lists(got, KR.knn(D, k, q_self), (N, q_self is None))
            c = index.counters()
            skipped = len(members) if q_self is not None else 0
            assert c["filtered"] + c["length_sum"] + c["dp"] == len(members) * N - skipped
            assert c["in_band"] == int((D <= w).sum()) - skipped
            assert c["steps_c1"] >= c["dp"] and c["steps_c2"] == c["steps_c9"] == 0
    finally:
        index.close()


# ---- 6. the device form on a side stream -------------------------------------------------------------------------------
def test_dev_form_on_a_side_stream(ctx):
    import torch
    w, k, key = 128, 8, "mod2"
    ts, ent, G = WC.store(key)
    trs, ents, _ = gpu_family(key)
    cap = 4096
    index = hs.PoSimilarityIndex(ts, ent, w, ctx=ctx, n_entities=G, max_queries=16, max_query_elems=cap, wide=True)
    try:
        side = torch.cuda.Stream()
        for sel in ([0, 3, 7, 12, 13, 14, 20, 21, 22, 29], [35, 5, 6, 30, 31, 23, 24, 25, 26, 27, 28, 1, 2, 4, 8, 9]):
            qts = hs.TraceSet([trs[i] for i in sel])
            q_ent = np.concatenate([ents[i] for i in sel])
            assert int(qts.off[-1]) <= cap
            q_self = np.array(sel, np.uint32)
            want = KR.knn(np.minimum(WC.matrices(key)[0][sel], w + 1), k, q_self)
            same_lists(index.query_csr(qts, q_ent, k, q_self), want, "host form")
            d_off = torch.from_numpy(qts.off.view(np.int64)).cuda()
            d_sym = torch.from_numpy(qts.sym.view(np.int64)).cuda()
            d_ent = torch.from_numpy(np.ascontiguousarray(q_ent).view(np.int32)).cuda()
            d_self = torch.from_numpy(q_self.view(np.int32)).cuda()
            d_keys = torch.full((len(sel) * k,), 7, dtype=torch.int64, device="cuda")
            torch.cuda.synchronize()  # the copies and the fill ran on torch's current stream
            index.query_dev(d_off.data_ptr(), d_sym.data_ptr(), d_ent.data_ptr(), d_self.data_ptr(), len(sel), k,
                            d_keys.data_ptr(), side.cuda_stream)
            side.synchronize()
            keys = d_keys.cpu().numpy().view(np.uint64).reshape(len(sel), k)
            assert np.array_equal((keys & np.uint64(0xFFFFFFFF)).astype(np.uint32), want[0])
            assert np.array_equal((keys >> np.uint64(32)).astype(np.uint32), want[1])
            c = index.counters(side.cuda_stream)
            assert c["filtered"] + c["length_sum"] + c["dp"] == len(sel) * (len(ts) - 1) and c["in_band"] >= 8
            assert c["steps_c1"] + c["steps_c2"] >= c["dp"] > 0
        # the guard: offsets that do not start at 0, decrease or pass max_query_elems write no list
        d_sym = torch.zeros(cap, dtype=torch.int64, device="cuda")
        d_ent = torch.zeros(cap, dtype=torch.int32, device="cuda")
        for offs in ([5, 10, 20], [0, 10, 5], [0, 10, cap + 5]):
            d_off = torch.tensor(offs, dtype=torch.int64, device="cuda")
            d_keys = torch.full((2 * k,), 7, dtype=torch.int64, device="cuda")
            torch.cuda.synchronize()
            index.query_dev(d_off.data_ptr(), d_sym.data_ptr(), d_ent.data_ptr(), 0, 2, k, d_keys.data_ptr(),
                            side.cuda_stream)
            side.synchronize()
            assert (d_keys.cpu().numpy().view(np.uint64) == np.uint64(2**64 - 1)).all(), offs
            with pytest.raises(_lib.NmzInvalidArgument, match=r"exceeded the plan's max_query_elems \(4096\)"):
                index.counters(side.cuda_stream)
    finally:
        index.close()


# ---- 7. the storage, and the gap this closes ---------------------------------------------------------------------------
def test_storage_finds_po_neighbours_beyond_band_64(ctx, tmp_path):
    """Four passing runs are random interleavings of three entities' fixed sequences of 100, 60 and 40 events; the
    two failing runs are further interleavings in which two neighbouring blocks of 40 (of 45) events of zk0 have
    changed places, so every failing-passing pair is 80 (90) PO-edits apart: beyond the narrow search's 64, within
    128. Before the wide search existed, DiffFailing(128, po=True, po_search=True) raised the library's refusal."""
    from test_align_po_gpu import _event, _interleave, same_profile
    from test_visualize import write_store
    rng = np.random.default_rng(78)
    seqs = [[_event("zk%d" % g, n) for n in range(L)] for g, L in enumerate((100, 60, 40))]
    tr = [_interleave(rng, seqs) for _ in range(4)]
    for blk in (40, 45):
        moved = list(seqs)
        moved[0] = seqs[0][:5] + seqs[0][5 + blk:5 + 2 * blk] + seqs[0][5:5 + blk] + seqs[0][5 + 2 * blk:]
        tr.append(_interleave(rng, moved))
    write_store(str(tmp_path), tr)
    for i in range(6):
        with open(os.path.join(str(tmp_path), "%08x" % i, "result.json"), "w") as f:
            json.dump({"successful": i < 4, "required_time": 1}, f)
    st = hs.LoadStorage(str(tmp_path))
    runs = st.traces()
    band, k = 128, 4
    ts, ent, names = hs.po_entities(runs)
    assert names == ["zk0", "zk1", "zk2"]
    part = lambda i: (ts.trace(i), ent[int(ts.off[i]):int(ts.off[i + 1])])
    host = {(i, j): po_slots(*part(i), *part(j), 3, band) for i in range(6) for j in range(6)}
    eight = np.array([[j, f] for f in (4, 5) for j in range(4)], np.uint32)
    want_d = [host[i, j][0] for i, j in eight.tolist()]
    assert want_d == [80] * 4 + [90] * 4  # beyond 64, within 128
    with pytest.raises(_lib.NmzInvalidArgument, match="NMZ_PO_KNN_MAX_BAND"):
        st.SearchSimilarPO(runs[4], 6, 65)
    # DiffFailing: the pairs and distances of the host forms, the profile of the host scripts
    prof = st.DiffFailing(band, k=k, ctx=ctx, po=True, po_search=True)
    assert prof.pairs.tolist() == eight.tolist()
    assert prof.dist.tolist() == want_d
    eh = hs.EditScripts(np.array(want_d, np.uint32), np.stack([host[i, j][1] for i, j in eight.tolist()]), band)
    same_profile(prof, hs.move_profile_of_wide(ts, eight, eh, host=True))
    # at band 64 the same call finds nothing: the narrow search lists every pair at 65
    none = st.DiffFailing(64, k=k, ctx=ctx, po=True, po_search=True)
    assert len(none.pairs) == 0
    # DiffSimilar: the failing run 4 against every stored run
    got = st.DiffSimilar(runs[4], k=6, band=band, po=True, po_search=True)
    order = sorted(range(6), key=lambda i: (host[i, 4][0], i))
    # itself, then the other failing run (its blocks of 45 against 40 are 25 PO-edits away), then the passing runs
    assert order == [4, 5, 0, 1, 2, 3] and [host[i, 4][0] for i in order] == [0, 25, 80, 80, 80, 80]
    assert [i for i, _, _ in got] == order
    for i, d, sc in got:
        assert d == host[i, 4][0] <= band
        assert sc.tobytes() == host[i, 4][1][:d].tobytes()
    # SearchSimilarPOWide: the host lexsort (the query is b of the host pairs' distance, which is symmetric)
    assert st.SearchSimilarPOWide(runs[4], 6, band) == [(i, host[i, 4][0]) for i in order]
    assert st.SearchSimilarPOWide(runs[4], 3, 8) == st.SearchSimilarPO(runs[4], 3, 8)
    with pytest.raises(TypeError):
        st.SearchSimilarPOWide(runs[4].symbols, 6, band)
