"""CPU: the PO k-NN search's filter and limits on the host (nmz_po_knn_bound_host, the refusals of nmz_po_knn*).

tests/po_knn_ref.py is DESIGN.md section 2, "PO k-NN search", in pure Python ints. The host form of the two lower
bounds is tied to it pair by pair and to three bucket values worked out by hand; the bounds are shown to be bounds
against nmz_ed_align_po_host's distances; and the filtered / DP / in-band counts that tests/test_po_knn_gpu.py expects
of the kernel's counters are made here, from the host forms alone. Every comparison is integer equality."""
import ctypes
import functools

import numpy as np
import pytest

import ed_cases as EC
import po_knn_ref as KR
from namazu_amd import _lib
from namazu_amd import historystorage as hs
from test_align_po_host import MAPS, ent_of, expected, gpu_family, po_slots, small_family

NONE = _lib.NMZ_NONE
# (filtered, through the filter, in band) over the 1,722 ordered pairs i != j of the 42-trace family
TABLE = {("mod2", 8): (1574, 148, 96), ("mod2", 32): (1498, 224, 200), ("mod2", 64): (1244, 478, 408),
         ("sparse", 8): (1570, 152, 142), ("sparse", 32): (1494, 228, 228), ("sparse", 64): (1110, 612, 612)}


# ---- 1. the bounds against the definition ----------------------------------------------------------------------------
def test_bucket_values_worked_by_hand():
    """mix(mix(prev + g) ^ cur) >> 57 run by hand in Python for three (g, prev, cur): a changed constant cannot pass
    by changing the reference and the library together. One element of entity g with symbol cur against the empty
    trace puts exactly that bucket at 1."""
    assert KR.mix(0) == 0 and KR.mix(1) == 0x5692161D100B05E5
    assert KR.bucket(0, KR.START, 1) == 79
    assert KR.bucket(5, 7, 9) == 43
    assert KR.bucket(1023, (1 << 64) - 1, 0x123456789ABCDEF0) == 9
    # through the library: the gram of [prev, cur] in entity g minus the gram of [prev] is the bucket of (prev, cur)
    for g, prev, cur in [(5, 7, 9), (1023, (1 << 64) - 1, 0x123456789ABCDEF0)]:
        b = KR.bucket(g, prev, cur)
        first = KR.bucket(g, KR.START, prev)
        lf, gram = KR.profile([prev, cur], [g, g])
        assert lf[g % 32] == 2 and gram[b] >= 1 and gram[first] >= 1 and sum(gram) == 2
        assert hs.po_knn_bounds([prev, cur], [g, g], [prev], [g], 1024) == (1, 1)
        assert hs.po_knn_bounds([prev, cur], [g, g], [], [], 1024) == (2, 1)
    assert hs.po_knn_bounds([1], [0], [], [], 1) == (1, 1)


@pytest.mark.parametrize("name", sorted(MAPS))
def test_bound_host_equals_definition(name):
    trs = small_family()
    ents = [ent_of(t, name)[0] for t in trs]
    G = MAPS[name][1]
    nonzero = 0
    for i, j in EC.all_ordered_pairs(len(trs)).tolist():
        want = KR.bounds(trs[i].tolist(), ents[i].tolist(), trs[j].tolist(), ents[j].tolist())
        assert hs.po_knn_bounds(trs[i], ents[i], trs[j], ents[j], G) == want, (name, i, j)
        nonzero += want[0] > 0 and want[1] > 0
    assert nonzero >= 40
    if name == "sparse":  # the NMZ_NONE elements count for nothing
        assert any((e == NONE).any() for e in ents)
        a, ea = trs[3], ents[3]
        keep = ea != NONE
        assert hs.po_knn_bounds(a, ea, a[keep], ea[keep], G) == (0, 0)


def test_saturation_and_folding():
    """300 equal grams saturate one bucket at 255 on both sides of the comparison; entities 1 and 33 share a lenfold
    word, so moving 5 elements between them leaves LB_len at 0."""
    a, b = [7] * 300, [7] * 256
    assert KR.bounds(a, [0] * 300, b, [0] * 256) == hs.po_knn_bounds(a, [0] * 300, b, [0] * 256, 1) == (44, 0)
    a, ea = list(range(10)), [1] * 10
    eb = [1] * 5 + [33] * 5
    got = hs.po_knn_bounds(a, ea, a, eb, 34)
    assert got == KR.bounds(a, ea, a, eb) and got[0] == 0 and got[1] >= 1


# ---- 2. the bound is a bound -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(MAPS))
def test_bound_is_a_bound_small_family(name):
    trs = small_family()
    ents = [ent_of(t, name)[0] for t in trs]
    G = MAPS[name][1]
    pairs = EC.all_ordered_pairs(len(trs)).tolist()
    lb = {(i, j): max(hs.po_knn_bounds(trs[i], ents[i], trs[j], ents[j], G)) for i, j in pairs}
    tight = filtered = 0
    for w in range(13):
        for i, j in pairs:
            d = po_slots(trs[i], ents[i], trs[j], ents[j], G, w)[0]
            if d <= w:
                assert lb[i, j] <= d, (name, w, i, j)
                tight += lb[i, j] == d and d > 0
            else:
                filtered += lb[i, j] > w
    assert tight >= 10 and filtered >= 100


@functools.lru_cache(maxsize=None)
def family_counts(name):
    """Over the 42-trace family under map `name`: D[42][42] = the PO distances from one band-1,024 host pass
    (NMZ_ALIGN_WIDE_MAX_BAND + 1 beyond it), LB[42][42] = max(LB_len, LB_gram) from the host form, LS[42][42] = the
    exact sum of the entities' length differences."""
    trs, ents, G = gpu_family(name)
    n = len(trs)
    pairs = EC.all_ordered_pairs(n)
    d, _ = expected(name, pairs, 1024)
    D = np.zeros((n, n), np.uint32)
    LB = np.zeros((n, n), np.uint64)
    LS = np.zeros((n, n), np.uint64)
    for (i, j), dist in zip(pairs.tolist(), d.tolist()):
        D[i, j] = dist
        LB[i, j] = max(hs.po_knn_bounds(trs[i], ents[i], trs[j], ents[j], G))
        LS[i, j] = KR.length_sum(ents[i], ents[j])
    return D, LB, LS


def expected_counters(name, w, self_excluded=True, no_filter=False):
    """The kernel's four counters for store = queries = the family at band w, from the host forms alone."""
    return counters_from(*family_counts(name), w, self_excluded=self_excluded, no_filter=no_filter)


def counters_from(D, LB, LS, w, self_excluded=True, no_filter=False):
    """The same from any family's matrices (tests/test_po_many_host.py has a second one)."""
    elig = ~np.eye(len(D), dtype=bool) if self_excluded else np.ones(D.shape, bool)
    filt = elig & (LB > w) & (not no_filter)
    lens = elig & ~filt & (LS > w)
    return {"filtered": int(filt.sum()), "length_sum": int(lens.sum()), "dp": int((elig & ~filt & ~lens).sum()),
            "in_band": int((elig & (D <= w)).sum())}


@pytest.mark.parametrize("name", ["mod2", "sparse"])
def test_bound_is_a_bound_gpu_family(name):
    D, LB, LS = family_counts(name)
    off = ~np.eye(len(D), dtype=bool)
    for w in (8, 32, 64):
        dw = np.minimum(D, w + 1)
        assert not ((dw <= w) & (LB > dw)).any() and not ((dw <= w) & (LS > dw)).any()
        got = (int((off & (LB > w)).sum()), int((off & (LB <= w)).sum()), int((off & (dw <= w)).sum()))
        print(name, w, "filtered / through the filter / in band", got)
        assert got == TABLE[name, w]
        c = expected_counters(name, w)
        assert (c["filtered"], c["length_sum"] + c["dp"], c["in_band"]) == TABLE[name, w]
    # the in-band counts of test_gpu_family_is_not_vacuous (the 42 self pairs included there)
    want = {"mod2": (138, 242, 450), "sparse": (184, 270, 654)}[name]
    assert tuple(int((D <= w).sum()) for w in (8, 32, 64)) == want
    if name == "mod2":  # pairs that pass the filter and end beyond the band: the DP's cut-off is exercised
        assert all(TABLE[name, w][1] - TABLE[name, w][2] >= 24 for w in (8, 32, 64))


# ---- 3. limits: each refusal with its message and no device ----------------------------------------------------------
def test_po_knn_refusals_need_no_device():
    L = _lib.load()
    P = _lib.ptr
    sym = np.arange(8, dtype=np.uint64)
    off = np.array([0, 3, 3, 8], np.uint64)
    ent = np.array([0, 1, NONE, 1, 1, 0, 3, 2], np.uint32)
    q_off = np.array([0, 2, 5], np.uint64)
    q_sym = np.arange(5, dtype=np.uint64)
    q_ent = np.array([0, 3, NONE, 2, 1], np.uint32)
    q_self = np.array([NONE, 2], np.uint32)
    ids = np.zeros((2, 64), np.uint32)
    ds = np.zeros((2, 64), np.uint32)

    def call(off=off, sym=sym, ent=ent, n_traces=3, G=4, q_off=q_off, q_sym=q_sym, q_ent=q_ent, q_self=q_self,
             n_queries=2, band=8, k=4, ids=ids, ds=ds):
        return L.nmz_po_knn(None, P(off), P(sym), P(ent), n_traces, G, P(q_off), P(q_sym), P(q_ent), P(q_self),
                            n_queries, band, k, P(ids), P(ds))

    plan = ctypes.c_void_p(1)

    def create(off=off, sym=sym, ent=ent, n_traces=3, G=4, band=8, max_queries=2, max_query_elems=5, opts=0):
        return L.nmz_po_knn_plan_create(None, P(off), P(sym), P(ent), n_traces, G, band, max_queries, max_query_elems,
                                        opts, ctypes.byref(plan))

    store = [
        ({}, "ctx is NULL"),
        ({"band": 0}, "ctx is NULL"),
        ({"band": 64, "G": 1024}, "ctx is NULL"),
        ({"band": 65}, "band 65 exceeds NMZ_PO_KNN_MAX_BAND (64): the PO search over wider bands is not built yet"),
        ({"G": 0}, "n_entities 0 must be 1 .. NMZ_PO_MAX_ENTITIES (1024)"),
        ({"G": 1025}, "n_entities 1025 must be 1 .. NMZ_PO_MAX_ENTITIES (1024)"),
        ({"G": 3}, "store element 6 has entity id 3: ids are < n_entities (3) or NMZ_NONE"),
        ({"n_traces": 2097152, "G": 1024}, "n_traces * n_entities = 2097152 * 1024 must stay below 2^31 - 1"),
        ({"off": np.array([0, 2**32 - 1, 2**32, 2**32], np.uint64)}, "store trace 0 has 4294967295 elements"),
        ({"off": np.array([0, 5, 3, 8], np.uint64)}, "store offsets must be non-decreasing (trace 1)"),
        ({"off": np.array([1, 3, 3, 8], np.uint64)}, "store offsets must start at 0"),
        ({"off": None}, "store offsets are NULL"),
        ({"sym": None}, "store sym is NULL"),
        ({"ent": None}, "store entity is NULL"),
        ({"band": 65, "G": 0}, "NMZ_PO_KNN_MAX_BAND"),  # the order: the band, then the entities, then the store
        ({"G": 0, "off": np.array([0, 5, 3, 8], np.uint64)}, "NMZ_PO_MAX_ENTITIES"),
    ]
    for fn in (call, create):
        for kw, msg in store:
            assert fn(**kw) == _lib.NMZ_EINVAL, kw
            assert msg in _lib.last_error(), (kw, _lib.last_error())
            assert fn is call or plan.value is None
            plan = ctypes.c_void_p(1)
    for kw, msg in [
        ({"k": 0}, "k 0 must be 1 .. NMZ_PO_KNN_MAX_K (64)"),
        ({"k": 65}, "k 65 must be 1 .. NMZ_PO_KNN_MAX_K (64)"),
        ({"band": 65, "k": 0}, "NMZ_PO_KNN_MAX_BAND"),
        ({"q_ent": np.array([0, 4, NONE, 2, 1], np.uint32)},
         "query element 1 has entity id 4: ids are < n_entities (4) or NMZ_NONE"),
        ({"G": 3}, "store element 6 has entity id 3"),  # the store before the queries
        ({"n_queries": 2097152, "G": 1024, "ent": np.zeros(8, np.uint32)},
         "n_queries * n_entities = 2097152 * 1024 must stay below 2^31 - 1"),
        ({"q_off": np.array([0, 2**32 - 1, 2**32], np.uint64)}, "query trace 0 has 4294967295 elements"),
        ({"q_off": np.array([0, 6, 5], np.uint64)}, "query offsets must be non-decreasing (trace 1)"),
        ({"q_off": np.array([2, 2, 5], np.uint64)}, "query offsets must start at 0"),
        ({"q_off": None}, "query offsets are NULL"),
        ({"q_sym": None}, "query sym is NULL"),
        ({"q_ent": None}, "query entity is NULL"),
        ({"q_self": np.array([NONE, 3], np.uint32)}, "q_self[1] = 3: a store index < n_traces (3) or NMZ_NONE"),
        ({"ids": None}, "knn_id or knn_dist is NULL"),
        ({"ds": None}, "knn_id or knn_dist is NULL"),
        ({"q_self": None}, "ctx is NULL"),  # legal: nothing is skipped
    ]:
        assert call(**kw) == _lib.NMZ_EINVAL, kw
        assert msg in _lib.last_error(), (kw, _lib.last_error())
    for kw, msg in [({"max_queries": 0}, "max_queries is 0"),
                    ({"max_queries": 2097152, "G": 1024, "ent": np.zeros(8, np.uint32)},
                     "max_queries * n_entities = 2097152 * 1024 must stay below 2^31 - 1"),
                    ({"opts": 4}, "opts 4: unknown bits")]:
        assert create(**kw) == _lib.NMZ_EINVAL, kw
        assert msg in _lib.last_error(), (kw, _lib.last_error())
    assert L.nmz_po_knn_plan_create(None, P(off), P(sym), P(ent), 3, 4, 8, 2, 5, 0, None) == _lib.NMZ_EINVAL
    assert "out is NULL" in _lib.last_error()
    # legal without a device: no query; no stored trace (all NMZ_NONE)
    assert call(n_queries=0, ids=None, ds=None) == _lib.NMZ_OK
    ids[:], ds[:] = 7, 7
    assert call(n_traces=0, q_self=None, k=64) == _lib.NMZ_OK
    assert (ids == NONE).all() and (ds == NONE).all()
    # the plan's other entry points
    assert L.nmz_po_knn_plan_destroy(None) == _lib.NMZ_OK
    for rc in (L.nmz_po_knn_query(None, P(q_off), P(q_sym), P(q_ent), None, 2, 4, P(ids), P(ds)),
               L.nmz_po_knn_query_dev(None, None, None, None, None, 0, 4, None, None),
               L.nmz_po_knn_counters(None, P(ids), None), L.nmz_po_knn_plan_info(None, None, None, None)):
        assert rc == _lib.NMZ_EINVAL and "plan is NULL" in _lib.last_error()
    assert (_lib.NMZ_PO_KNN_MAX_BAND, _lib.NMZ_PO_KNN_MAX_K, _lib.NMZ_PO_KNN_OPT_NO_FILTER) == (64, 64, 1)


def test_bound_host_refusals():
    L = _lib.load()
    P = _lib.ptr
    a = np.arange(3, dtype=np.uint64)
    e = np.array([0, 1, NONE], np.uint32)
    bad = np.array([0, 2, NONE], np.uint32)
    x, y = ctypes.c_uint32(), ctypes.c_uint32()
    for args, msg in [
        ((P(a), P(e), 2**32 - 1, P(a), P(e), 3, 2, ctypes.byref(x), ctypes.byref(y)), "a has 4294967295 elements"),
        ((P(a), P(e), 3, P(a), P(e), 2**32 - 1, 2, ctypes.byref(x), ctypes.byref(y)), "b has 4294967295 elements"),
        ((P(a), None, 3, P(a), P(e), 3, 2, ctypes.byref(x), ctypes.byref(y)), "a, b or an entity array is NULL"),
        ((P(a), P(e), 3, P(a), P(e), 3, 2, None, ctypes.byref(y)), "lb_len or lb_gram is NULL"),
        ((P(a), P(e), 3, P(a), P(e), 3, 0, ctypes.byref(x), ctypes.byref(y)), "NMZ_PO_MAX_ENTITIES (1024)"),
        ((P(a), P(bad), 3, P(a), P(e), 3, 2, ctypes.byref(x), ctypes.byref(y)), "a's element 1 has entity id 2"),
        ((P(a), P(e), 3, P(a), P(bad), 3, 2, ctypes.byref(x), ctypes.byref(y)), "b's element 1 has entity id 2"),
    ]:
        assert L.nmz_po_knn_bound_host(*args) == _lib.NMZ_EINVAL, msg
        assert msg in _lib.last_error(), (msg, _lib.last_error())
    assert L.nmz_po_knn_bound_host(None, None, 0, None, None, 0, 1, ctypes.byref(x), ctypes.byref(y)) == _lib.NMZ_OK
    assert (x.value, y.value) == (0, 0)


# ---- 4. the Python surface -------------------------------------------------------------------------------------------
def test_po_search_needs_po(tmp_path):
    st = hs.Naive(str(tmp_path))
    with pytest.raises(ValueError, match="po_search=True needs po=True"):
        st.DiffFailing(8, po_search=True)
    with pytest.raises(ValueError, match="po_search=True needs po=True"):
        st.DiffSimilar(hs.SingleTrace([1, 2], entities=["a", "b"]), 4, 8, po_search=True)


def test_python_refusals_need_no_device():
    ts = hs.TraceSet([np.arange(3, dtype=np.uint64), np.arange(4, dtype=np.uint64)])
    ent = np.array([0, 1, NONE, 1, 1, 0, 1], np.uint32)
    with pytest.raises(_lib.NmzInvalidArgument, match="NMZ_PO_KNN_MAX_BAND"):
        hs.po_knn(ts, ent, ts, ent, 4, 65)
    with pytest.raises(_lib.NmzInvalidArgument, match="NMZ_PO_KNN_MAX_K"):
        hs.po_knn(ts, ent, ts, ent, 65, 8, ctx=None)
    with pytest.raises(_lib.NmzInvalidArgument, match="NMZ_PO_KNN_MAX_BAND"):
        hs.PoSimilarityIndex(ts, ent, 65, ["a", "b"])
    with pytest.raises(_lib.NmzInvalidArgument, match="NMZ_PO_MAX_ENTITIES"):
        hs.PoSimilarityIndex(ts, ent, 8, ["e%d" % i for i in range(1024)])
    ids, ds = hs.po_knn(ts, ent, hs.TraceSet([]), np.zeros(1, np.uint32), 4, 8)
    assert ids.shape == ds.shape == (0, 4)
    ids, ds = hs.po_knn(hs.TraceSet([]), np.zeros(1, np.uint32), ts, ent, 3, 8, n_entities=2)
    assert ids.shape == (2, 3) and (ids == NONE).all() and (ds == NONE).all()
