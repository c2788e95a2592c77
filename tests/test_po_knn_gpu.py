"""GPU: the PO k-NN search (k_po_knn_profile, k_po_knn, k_po_knn_fill; the nmz_po_knn* entry points;
PoSimilarityIndex, Naive.SearchSimilarPO and the po_search keyword of DiffSimilar / DiffFailing) against the host
forms: nmz_ed_align_po_host for the distances, tests/po_knn_ref.py for the lists, and the counts that
tests/test_po_knn_host.py makes from nmz_po_knn_bound_host for the kernel's four counters.

Every id and distance of every list is compared. The shapes are the smallest at which these kernels can still go
wrong: the bands on both sides of the joints of the cells per lane (31 / 32, 63 / 64) and band 0, k = 1 and k past
the store's size, stores of 1, 63, 64, 65 and 129 traces around the 64-candidate blocks, dozens of ties, the two
ends of the id range, one plan on a side stream twice."""
import json
import os

import numpy as np
import pytest

import align_ref as AR
import ed_cases as EC
import po_knn_ref as KR
import po_ref as PR
from namazu_amd import _lib
from namazu_amd import historystorage as hs
from test_align_po_host import gpu_family, interleavings, po_slots
from test_po_knn_host import expected_counters, family_counts

pytestmark = pytest.mark.gpu

NONE = _lib.NMZ_NONE
BANDS = (0, 8, 31, 32, 63, 64)


def family_store(name):
    trs, ents, G = gpu_family(name)
    return hs.TraceSet(list(trs)), np.concatenate(ents), G


def same_lists(got, want, what):
    assert np.array_equal(got[0], want[0]), what
    assert np.array_equal(got[1], want[1]), what


# ---- 1. the family against the host ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["mod2", "sparse"])
def test_family(ctx, name):
    """Store = queries = the 42 traces. k = 64 > 41 checks the NMZ_NONE tail; q_self = NULL lets each trace find
    itself at 0 first. The counters equal the counts made on the CPU."""
    ts, ent, G = family_store(name)
    n = len(ts)
    D = family_counts(name)[0]
    filtered = dp = beyond = 0
    for w in BANDS:
        Dw = np.minimum(D, w + 1)
        index = hs.PoSimilarityIndex(ts, ent, w, ctx=ctx, n_entities=G, max_queries=64,
                                     max_query_elems=int(ts.off[-1]))
        try:
            for k in (1, 8, 64):
                for q_self in (np.arange(n, dtype=np.uint32), None):
                    got = index.query_csr(ts, ent, k, q_self)
                    same_lists(got, KR.knn(Dw, k, q_self), (name, w, k, q_self is None))
                    c = index.counters()
                    assert c == expected_counters(name, w, self_excluded=q_self is not None), (name, w, k)
                    if k == 64:
                        assert (got[0][:, n - (q_self is not None):] == NONE).all()
            filtered += c["filtered"]
            dp += c["dp"]
            beyond += c["dp"] - c["in_band"]
            if w >= 8:
                assert c["filtered"] >= 16 and c["dp"] >= 16 and (name != "mod2" or c["dp"] - c["in_band"] >= 16)
            assert index.info()[0] > 0 and index.info()[1] >= 1
        finally:
            index.close()
    assert filtered >= 16 and dp >= 16 and (name != "mod2" or beyond >= 16)
    # the one-shot entry point: the same lists
    Dw = np.minimum(D, 33)
    same_lists(hs.po_knn(ts, ent, ts, ent, 8, 32, n_entities=G, q_self=np.arange(n, dtype=np.uint32), ctx=ctx),
               KR.knn(Dw, 8, np.arange(n)), name)


# ---- 2. the filter off -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["mod2", "sparse"])
def test_filter_off(ctx, name):
    w = 32
    ts, ent, G = family_store(name)
    n = len(ts)
    q_self = np.arange(n, dtype=np.uint32)
    Dw = np.minimum(family_counts(name)[0], w + 1)
    lists = {}
    for opts in (0, _lib.NMZ_PO_KNN_OPT_WHOLE_BLOCKS, _lib.NMZ_PO_KNN_OPT_NO_FILTER | _lib.NMZ_PO_KNN_OPT_WHOLE_BLOCKS,
                 _lib.NMZ_PO_KNN_OPT_NO_FILTER):
        index = hs.PoSimilarityIndex(ts, ent, w, ctx=ctx, n_entities=G, max_queries=64,
                                     max_query_elems=int(ts.off[-1]), opts=opts)
        try:
            lists[opts] = index.query_csr(ts, ent, 64, q_self)
            c = index.counters()
            assert c == expected_counters(name, w, no_filter=bool(opts & _lib.NMZ_PO_KNN_OPT_NO_FILTER))
            assert index.info()[1] == (n if opts & _lib.NMZ_PO_KNN_OPT_WHOLE_BLOCKS else 64 * n)  # items = workgroups
        finally:
            index.close()
    assert c["filtered"] == 0 and c["length_sum"] + c["dp"] == n * (n - 1) and c["length_sum"] >= 16
    for opts in (1, 2, 3):
        assert lists[0][0].tobytes() == lists[opts][0].tobytes() and lists[0][1].tobytes() == lists[opts][1].tobytes()
    same_lists(lists[1], KR.knn(Dw, 64, q_self), name)


# ---- 3. one entity ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", [8, 64])
def test_one_entity_equals_the_exact_search(ctx, w):
    """n_entities = 1: nmz_ed_plan_query_knn's lists (SimilarityIndex.query) and the host's. The family's lengths 0,
    1, 63, 64, 65, 127, 128, 129 sit on the 64-row staging joints."""
    trs = gpu_family("mod2")[0]
    ts = hs.TraceSet(list(trs))
    n = len(ts)
    ent = np.zeros(int(ts.off[-1]), np.uint32)
    D = np.array([[po_slots(trs[i], ent[:len(trs[i])], trs[j], ent[:len(trs[j])], 1, w)[0] for j in range(n)]
                  for i in range(n)], np.uint32)
    assert (D <= w).sum() >= 42 + 16 and (D > w).sum() >= 16
    index = hs.PoSimilarityIndex(ts, ent, w, ctx=ctx, n_entities=1, max_queries=64, max_query_elems=int(ts.off[-1]))
    exact = hs.SimilarityIndex(ts, w, ctx=ctx)
    try:
        for k in (8, 64):
            got = index.query_csr(ts, ent, k)
            same_lists(got, KR.knn(D, k), (w, k))
            same_lists(got, exact.query(list(trs), k), (w, k, "SimilarityIndex"))
    finally:
        index.close()
        exact.close()


# ---- 4. candidate-block joints and ties ------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 63, 64, 65, 129])
def test_candidate_blocks_and_ties(ctx, N):
    """Interleavings of three entities' fixed sequences: dozens of candidates tie at 0 and at 1 .. 4, so the id
    order decides; dist == 0 <=> equal in partial order (first_equal)."""
    w, k = 4, 64
    trs = interleavings(np.random.default_rng(1000 + N), N - 8 if N > 8 else N, 8 if N > 8 else 0,
                        lens=(40, 64, 70))
    singles = [hs.SingleTrace(s, entities=["e%d" % g for g in e]) for s, e in trs]
    ts, ent, names = hs.po_entities(singles)
    assert len(names) == 3
    members = sorted({0, N // 3, N // 2, N - 1})
    D = np.array([[po_slots(trs[m][0], trs[m][1], s, e, 3, w)[0] for s, e in trs] for m in members], np.uint32)
    fe = hs.first_equal(singles, po_reduction=True, ctx=ctx)
    assert np.array_equal(D == 0, fe[members][:, None] == fe[None, :])
    if N > 8:
        assert (D == 0).sum() >= N - 8 and ((D >= 1) & (D <= w)).sum() >= 8
    index = hs.PoSimilarityIndex(ts, ent, w, names, ctx=ctx)
    try:
        queries = [singles[m] for m in members]
        for q_self in (np.array(members, np.uint32), None):
            got = index.query(queries, k, q_self)
            same_lists(got, KR.knn(D, k, q_self), (N, q_self is None))
            c = index.counters()
            assert c["filtered"] + c["length_sum"] + c["dp"] == len(members) * N - (len(members) if q_self is not None
                                                                                   else 0)
            assert c["in_band"] == int((D <= w).sum()) - (len(members) if q_self is not None else 0)
    finally:
        index.close()


# ---- 5. the id range -------------------------------------------------------------------------------------------------
def test_ends_of_the_id_range_and_none(ctx):
    """n_entities = 1,024 with ids 0 and 1,023 only, 20 % of the elements NMZ_NONE, against the host."""
    w, k, G = 32, 8, 1024
    rng = np.random.default_rng(5)
    trs = gpu_family("mod2")[0][:24]
    ents = []
    for t in trs:
        e = np.where((t % np.uint64(2)) == 0, 0, 1023).astype(np.uint32)
        e[rng.random(len(t)) < 0.2] = NONE
        ents.append(e)
    ts, ent = hs.TraceSet(list(trs)), np.concatenate(ents)
    n = len(ts)
    assert (ent == NONE).sum() >= 100 and set(np.unique(ent).tolist()) == {0, 1023, NONE}
    D = np.array([[po_slots(trs[i], ents[i], trs[j], ents[j], G, w)[0] for j in range(n)] for i in range(n)], np.uint32)
    assert ((D <= w) & ~np.eye(n, dtype=bool)).sum() >= 16 and (D > w).sum() >= 16
    q_self = np.arange(n, dtype=np.uint32)
    same_lists(hs.po_knn(ts, ent, ts, ent, k, w, n_entities=G, q_self=q_self, ctx=ctx), KR.knn(D, k, q_self), "1024")


def test_entities_the_store_lacks(ctx):
    """A query's entities unknown to the store share the spare id: the distance po_ref.script gives with every
    entity on an id of its own."""
    w = 8
    store = [hs.SingleTrace([10, 11, 20, 12], entities=["a", "a", "b", "a"]),
             hs.SingleTrace([10, 20, 21, 11], entities=["a", "b", "b", "a"]),
             hs.SingleTrace([], entities=[])]
    query = hs.SingleTrace([30, 10, 40, 11, 20, 31, 12], entities=["c", "a", "d", "a", "b", "c", "a"])
    ts, ent, names = hs.po_entities(store)
    assert names == ["a", "b"]
    real = {"a": 0, "b": 1, "c": 2, "d": 3}
    want = [PR.script(query.symbols.tolist(), [real[e] for e in query.entities], s.symbols.tolist(),
                      [real[e] for e in s.entities], w)[0] for s in store]
    assert want == [3, 5, 7]
    index = hs.PoSimilarityIndex(ts, ent, w, names, ctx=ctx)
    try:
        assert index.n_entities == 3 and index.query_inputs([query])[1].tolist() == [2, 0, 2, 0, 1, 2, 0]
        ids, ds = index.query([query], 3)
        assert ids.tolist() == [[0, 1, 2]] and ds.tolist() == [want]
    finally:
        index.close()


# ---- 6. the device form on a side stream -----------------------------------------------------------------------------
def test_dev_form_on_a_side_stream(ctx):
    import torch
    w, k, name = 32, 8, "mod2"
    ts, ent, G = family_store(name)
    trs, ents, _ = gpu_family(name)
    cap = 4096
    index = hs.PoSimilarityIndex(ts, ent, w, ctx=ctx, n_entities=G, max_queries=16, max_query_elems=cap)
    try:
        side = torch.cuda.Stream()
        for sel in ([0, 3, 7, 12, 13, 14, 20, 21, 22, 29], [35, 5, 6, 30, 31, 23, 24, 25, 26, 27, 28, 1, 2, 4, 8, 9]):
            qts = hs.TraceSet([trs[i] for i in sel])
            q_ent = np.concatenate([ents[i] for i in sel])
            assert int(qts.off[-1]) <= cap
            q_self = np.array(sel, np.uint32)
            want = index.query_csr(qts, q_ent, k, q_self)
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
        with pytest.raises(_lib.NmzInvalidArgument, match=r"n_queries 17 exceeds the plan's max_queries \(16\)"):
            index.query_dev(d_off.data_ptr(), d_sym.data_ptr(), d_ent.data_ptr(), d_self.data_ptr(), 17, k,
                            d_keys.data_ptr(), side.cuda_stream)
        assert "max_query_elems is 4096" in _lib.last_error()
        index.query_dev(0, 0, 0, 0, 0, k, 0, side.cuda_stream)  # no query: nothing is enqueued
        # offsets that pass max_query_elems stay inside the plan's scratch, and the search writes no list
        d_off = torch.tensor([0, 10, cap + 5], dtype=torch.int64, device="cuda")
        d_sym = torch.zeros(cap, dtype=torch.int64, device="cuda")
        d_ent = torch.zeros(cap, dtype=torch.int32, device="cuda")
        d_keys = torch.full((2 * k,), 7, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        index.query_dev(d_off.data_ptr(), d_sym.data_ptr(), d_ent.data_ptr(), 0, 2, k, d_keys.data_ptr(),
                        side.cuda_stream)
        side.synchronize()
        assert (d_keys.cpu().numpy().view(np.uint64) == np.uint64(2**64 - 1)).all()
        with pytest.raises(_lib.NmzInvalidArgument, match=r"exceeded the plan's max_query_elems \(4096\)"):
            index.counters(side.cuda_stream)
    finally:
        index.close()


def test_host_form_batches_by_the_plans_capacity(ctx):
    """max_queries = 5 and max_query_elems just above the longest query: the 42 queries run in many batches, with the
    same lists; a plan too small for one query is refused with both numbers."""
    w, k, name = 8, 4, "sparse"
    ts, ent, G = family_store(name)
    Dw = np.minimum(family_counts(name)[0], w + 1)
    index = hs.PoSimilarityIndex(ts, ent, w, ctx=ctx, n_entities=G, max_queries=5, max_query_elems=1600)
    try:
        same_lists(index.query_csr(ts, ent, k), KR.knn(Dw, k), "batches")
        ids = np.zeros((len(ts), k), np.uint32)
        small = hs.PoSimilarityIndex(ts, ent, w, ctx=ctx, n_entities=G, max_queries=5, max_query_elems=100)
        try:
            rc = _lib.load().nmz_po_knn_query(small.plan, _lib.ptr(ts.off), _lib.ptr(ts.sym), _lib.ptr(ent), None,
                                              len(ts), k, _lib.ptr(ids), _lib.ptr(ids.copy()))
            assert rc == _lib.NMZ_EINVAL
            lens = np.diff(ts.off).astype(np.int64)
            first = int(np.argmax(lens > 100))
            assert "query %d has %d elements: more than the plan's max_query_elems (100)" % (first, lens[first]) in \
                _lib.last_error()
        finally:
            small.close()
    finally:
        index.close()


# ---- 7. the storage, and the gap this closes -------------------------------------------------------------------------
def test_storage_finds_po_neighbours_beyond_the_exact_band(ctx, tmp_path):
    """Four passing runs are random interleavings of three entities' fixed sequences of 24, 20 and 16 events; the two
    failing runs are two more interleavings in which one event of zk1 is delivered three places later within its
    entity. Every failing-passing pair is tens of exact edits apart, so at band 8 the exact search finds nothing;
    the PO search finds all of them at 2."""
    from test_align_po_gpu import _event, _interleave, same_profile
    from test_visualize import write_store
    rng = np.random.default_rng(77)
    seqs = [[_event("zk%d" % g, n) for n in range(L)] for g, L in enumerate((24, 20, 16))]
    moved = list(seqs)
    moved[1] = seqs[1][:3] + seqs[1][4:7] + [seqs[1][3]] + seqs[1][7:]
    tr = [_interleave(rng, seqs) for _ in range(4)] + [_interleave(rng, moved) for _ in range(2)]
    write_store(str(tmp_path), tr)
    for i in range(6):
        with open(os.path.join(str(tmp_path), "%08x" % i, "result.json"), "w") as f:
            json.dump({"successful": i < 4, "required_time": 1}, f)
    st = hs.LoadStorage(str(tmp_path))
    runs = st.traces()
    band, k = 8, 4
    x = int(runs[4].symbols[[e["option"]["seq"] == 3 and e["entity"] == "zk1" for e in tr[4][1]].index(True)])
    eight = np.array([[j, f] for f in (4, 5) for j in range(4)], np.uint32)
    # the parent's behaviour, which stays: the exact search at the band finds no neighbour
    exact = hs.ed_pairs(hs.TraceSet([r.symbols for r in runs]), eight, 64, ctx=ctx)
    print("exact distances", exact.tolist())
    assert (exact >= 40).all() and (exact <= 52).all()
    assert (hs.ed_pairs(hs.TraceSet([r.symbols for r in runs]), eight, band, ctx=ctx) == band + 1).all()
    none = st.DiffFailing(band, k=k, ctx=ctx, po=True)
    assert len(none.pairs) == 0 and int(none.info["n_scripts"]) == 0 and int(none.info["n_ops"]) == 0
    # the PO search
    prof = st.DiffFailing(band, k=k, ctx=ctx, po=True, po_search=True)
    assert prof.pairs.tolist() == eight.tolist()
    assert prof.dist.tolist() == [2] * 8
    top = prof.top(1)
    assert len(top) == 1 and top[0][0] == x and top[0][1]["later"] == 8 and top[0][1]["n_pairs"] == 8
    ts, ent, names = hs.po_entities(runs)
    assert names == ["zk0", "zk1", "zk2"]
    slots = [po_slots(ts.trace(i), ent[int(ts.off[i]):int(ts.off[i + 1])], ts.trace(j),
                      ent[int(ts.off[j]):int(ts.off[j + 1])], 3, band) for i, j in eight.tolist()]
    eh = hs.EditScripts(np.array([d for d, _ in slots], np.uint32), np.stack([o for _, o in slots]), band)
    same_profile(prof, hs.move_profile_of_wide(ts, eight, eh, host=True))
    # DiffSimilar: the failing run 4 against every stored run
    assert [i for i, _, _ in st.DiffSimilar(runs[4], k=6, band=band, po=True)] == [4]  # the exact search: itself
    got = st.DiffSimilar(runs[4], k=6, band=band, po=True, po_search=True)
    assert [i for i, _, _ in got] == [4, 5, 0, 1, 2, 3]
    by_id = {i: (d, sc) for i, d, sc in got}
    assert by_id[4][0] == 0 and by_id[5][0] == 0 and len(by_id[4][1]) == 0 and len(by_id[5][1]) == 0
    for i in range(4):
        d, sc = by_id[i]
        assert d == 2 and [int(o["kind"]) for o in sc] == [AR.DEL, AR.INS]
        assert int(runs[i].symbols[sc[0]["a_pos"]]) == x and int(runs[4].symbols[sc[1]["b_pos"]]) == x
    assert st.SearchSimilarPO(runs[4], 6, band) == [(4, 0), (5, 0), (0, 2), (1, 2), (2, 2), (3, 2)]
    with pytest.raises(_lib.NmzInvalidArgument, match="NMZ_PO_KNN_MAX_BAND"):
        st.SearchSimilarPO(runs[4], 6, 65)
    with pytest.raises(TypeError):
        st.SearchSimilarPO(runs[4].symbols, 6, band)
