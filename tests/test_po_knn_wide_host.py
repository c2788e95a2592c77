"""CPU: the wide PO k-NN search's limits and its test inputs (the refusals of nmz_po_knn_wide*, the "cut" family of
tests/po_knn_wide_cases.py).

The refusal table is tests/test_po_knn_host.py's with the band line at 1,025 and opts bit 8 unknown: every limit,
message and order of checks of the wide entry points is the narrow form's. The family's conditions -- what makes the
GPU test of k_po_knn_wide's budget cut-off not vacuous -- are asserted here from the host forms alone, and the two
lower bounds are shown to be bounds at the ten joint bands over both families. Every comparison is integer
equality."""
import ctypes

import numpy as np
import pytest

import po_knn_wide_cases as WC
from namazu_amd import _lib
from namazu_amd import historystorage as hs

NONE = _lib.NMZ_NONE


# ---- 1. limits: each refusal with its message and no device ----------------------------------------------------------
def test_po_knn_wide_refusals_need_no_device():
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
             n_queries=2, band=128, k=4, ids=ids, ds=ds):
        return L.nmz_po_knn_wide(None, P(off), P(sym), P(ent), n_traces, G, P(q_off), P(q_sym), P(q_ent), P(q_self),
                                 n_queries, band, k, P(ids), P(ds))

    plan = ctypes.c_void_p(1)

    def create(off=off, sym=sym, ent=ent, n_traces=3, G=4, band=128, max_queries=2, max_query_elems=5, opts=0):
        return L.nmz_po_knn_wide_plan_create(None, P(off), P(sym), P(ent), n_traces, G, band, max_queries,
                                             max_query_elems, opts, ctypes.byref(plan))

    store = [
        ({}, "ctx is NULL"),
        ({"band": 0}, "ctx is NULL"),
        ({"band": 64}, "ctx is NULL"),
        ({"band": 65}, "ctx is NULL"),
        ({"band": 1024, "G": 1024}, "ctx is NULL"),
        ({"band": 1025},
         "band 1025 exceeds NMZ_PO_KNN_WIDE_MAX_BAND (1024): the PO search over wider bands is not built yet"),
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
        ({"band": 1025, "G": 0}, "NMZ_PO_KNN_WIDE_MAX_BAND"),  # the order: the band, the entities, then the store
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
        ({"band": 1025, "k": 0}, "NMZ_PO_KNN_WIDE_MAX_BAND"),
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
                    ({"opts": 8}, "opts 8: unknown bits"),
                    ({"opts": 4}, "ctx is NULL"),  # NMZ_PO_KNN_OPT_FULL_BAND: the wide create knows it
                    ({"opts": 7, "band": 8}, "ctx is NULL")]:
        assert create(**kw) == _lib.NMZ_EINVAL, kw
        assert msg in _lib.last_error(), (kw, _lib.last_error())
    assert L.nmz_po_knn_wide_plan_create(None, P(off), P(sym), P(ent), 3, 4, 128, 2, 5, 0, None) == _lib.NMZ_EINVAL
    assert "out is NULL" in _lib.last_error()
    # legal without a device: no query; no stored trace (all NMZ_NONE)
    assert call(n_queries=0, ids=None, ds=None) == _lib.NMZ_OK
    ids[:], ds[:] = 7, 7
    assert call(n_traces=0, q_self=None, k=64) == _lib.NMZ_OK
    assert (ids == NONE).all() and (ds == NONE).all()
    # the narrow create keeps its band and its opts
    assert L.nmz_po_knn_plan_create(None, P(off), P(sym), P(ent), 3, 4, 65, 2, 5, 0, ctypes.byref(plan)) == \
        _lib.NMZ_EINVAL and "NMZ_PO_KNN_MAX_BAND (64)" in _lib.last_error()
    assert L.nmz_po_knn_plan_create(None, P(off), P(sym), P(ent), 3, 4, 8, 2, 5, 4, ctypes.byref(plan)) == \
        _lib.NMZ_EINVAL and "opts 4: unknown bits" in _lib.last_error()


def test_wide_counters_refuse_a_null_plan_and_the_constants():
    L = _lib.load()
    out = np.zeros(_lib.NMZ_PO_KNN_WIDE_NCOUNTERS, np.uint64)
    assert L.nmz_po_knn_wide_counters(None, _lib.ptr(out), None) == _lib.NMZ_EINVAL
    assert "plan is NULL" in _lib.last_error()
    assert (_lib.NMZ_PO_KNN_WIDE_MAX_BAND, _lib.NMZ_PO_KNN_WIDE_NCOUNTERS, _lib.NMZ_PO_KNN_OPT_FULL_BAND) == \
        (1024, 9, 4)
    assert _lib.NMZ_PO_KNN_MAX_BAND == 64 and len(hs.PoSimilarityIndex.STEP_NAMES) == 5
    # the header says the same
    import os
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include",
                             "nmz_gpu.h")).read()
    for line in ("#define NMZ_PO_KNN_WIDE_MAX_BAND 1024", "#define NMZ_PO_KNN_WIDE_NCOUNTERS 9",
                 "#define NMZ_PO_KNN_OPT_FULL_BAND 4u", "#define NMZ_PO_KNN_MAX_BAND 64"):
        assert line in text, line


# ---- 2. the second family's conditions -------------------------------------------------------------------------------
def test_cut_family_conditions():
    """What the family is for, from the host forms alone: at every joint band pairs that pass both filters and end
    beyond the band, pairs in band above 64, pairs ended by the per-entity length check, and at band 1,024 every
    cell count."""
    trs, ents, G = WC.family("cut")
    assert len(trs) == 28 and G == 5 and sum(len(t) for t in trs) < 90000
    D = WC.matrices("cut")[0]
    by_length = 0
    for w in WC.BANDS:
        elig, filt, lens, dp = WC.pair_classes("cut", w)
        beyond = int((dp & (D > w)).sum())
        mid = int((elig & (D <= w) & (D > 64)).sum())
        ends = [WC.walk("cut", i, j, w)[1] for i, j in np.argwhere(dp).tolist()]
        print(w, "filtered", int(filt.sum()), "length sum", int(lens.sum()), "dp", int(dp.sum()), "beyond after a dp",
              beyond, "in band above 64", mid, "ended by a length check", ends.count("length"))
        assert beyond >= 16
        assert ends.count("dp") + ends.count("length") == beyond
        if w != 65:
            assert mid >= 16
        by_length += ends.count("length")
    assert by_length >= 16
    # band 65's in-band pairs above 64 come from the 42-trace family under mod2
    D42 = WC.matrices("mod2")[0]
    assert int((D42 == 65).sum()) == 62
    c = WC.expected_counters("cut", 1024)
    print(c)
    assert all(c[name] > 0 for name in hs.PoSimilarityIndex.STEP_NAMES)
    assert all(v == 0 for name, v in WC.expected_counters("cut", 64).items() if name.startswith("steps"))
    full = WC.expected_counters("cut", 256, full_band=True)
    assert full["steps_c3"] == sum(v for name, v in WC.expected_counters("cut", 256).items()
                                   if name.startswith("steps")) > 0
    assert full["steps_c1"] == full["steps_c2"] == full["steps_c5"] == full["steps_c9"] == 0


def test_cells_are_the_layouts_joints():
    assert [WC.cells(w) for w in (0, 65, 127, 128, 255, 256, 383, 384, 639, 640, 1024)] == \
        [1, 1, 1, 2, 2, 3, 3, 5, 5, 9, 9]
    for c, top in zip((1, 2, 3, 5), (127, 255, 383, 639)):
        assert 2 * top + 1 <= 256 * c < 2 * (top + 1) + 1  # the widest band that c cells per thread hold


# ---- 3. the bound is a bound at the wide bands -----------------------------------------------------------------------
@pytest.mark.parametrize("key", ["cut", "mod2", "sparse"])
def test_bounds_never_exceed_an_in_band_distance(key):
    D, LB, LS, _, _ = WC.matrices(key)
    off = ~np.eye(len(D), dtype=bool)
    filtered = 0
    for w in WC.BANDS:
        dw = np.minimum(D, w + 1)
        assert not (off & (dw <= w) & (LB > dw)).any() and not (off & (dw <= w) & (LS > dw)).any()
        filtered += int((off & (LB > w)).sum())
    assert filtered >= 16


# ---- 4. the Python surface -------------------------------------------------------------------------------------------
def test_python_refusals_need_no_device():
    ts = hs.TraceSet([np.arange(3, dtype=np.uint64), np.arange(4, dtype=np.uint64)])
    ent = np.array([0, 1, NONE, 1, 1, 0, 1], np.uint32)
    with pytest.raises(_lib.NmzInvalidArgument, match="NMZ_PO_KNN_WIDE_MAX_BAND"):
        hs.po_knn_wide(ts, ent, ts, ent, 4, 1025)
    with pytest.raises(_lib.NmzInvalidArgument, match="NMZ_PO_KNN_MAX_K"):
        hs.po_knn_wide(ts, ent, ts, ent, 65, 128, ctx=None)
    with pytest.raises(_lib.NmzInvalidArgument, match="NMZ_PO_KNN_WIDE_MAX_BAND"):
        hs.PoSimilarityIndex(ts, ent, 1025, ["a", "b"], wide=True)
    with pytest.raises(_lib.NmzInvalidArgument, match="NMZ_PO_MAX_ENTITIES"):
        hs.PoSimilarityIndex(ts, ent, 128, ["e%d" % i for i in range(1024)], wide=True)
    # the narrow forms keep refusing band 65
    with pytest.raises(_lib.NmzInvalidArgument, match=r"NMZ_PO_KNN_MAX_BAND \(64\)"):
        hs.po_knn(ts, ent, ts, ent, 4, 65)
    with pytest.raises(_lib.NmzInvalidArgument, match=r"NMZ_PO_KNN_MAX_BAND \(64\)"):
        hs.PoSimilarityIndex(ts, ent, 65, ["a", "b"])
    ids, ds = hs.po_knn_wide(ts, ent, hs.TraceSet([]), np.zeros(1, np.uint32), 4, 128)
    assert ids.shape == ds.shape == (0, 4)
    ids, ds = hs.po_knn_wide(hs.TraceSet([]), np.zeros(1, np.uint32), ts, ent, 3, 1024, n_entities=2)
    assert ids.shape == (2, 3) and (ids == NONE).all() and (ds == NONE).all()
