"""GPU: the PO kernels at hundreds of populated entities -- K10 (k_po_project, k_po_subpairs, k_po_gather over the
aligners) and K11 (k_po_knn_profile, k_po_knn, k_po_knn_fill) on the family of tests/po_many_cases.py: 68 traces over
200 populated entities, under n_entities = 1,024 (ids on the joints of the kernels' layouts) and under n_entities =
203 (ranks: a partial last chunk of 64, one populated wave of k_po_gather, up to 64 distinct ids in 64 elements).

The projection is compared with numpy, the scripts slot for slot with nmz_ed_align_po_host, the profile with
nmz_move_profile_wide_host over the host scripts, the lists with tests/po_knn_ref.py over the host distances and the
kernel's counters with the counts made from the host bounds; tests/test_po_many_host.py ties those host forms to the
definition on this family and asserts what the family exercises: a budget carried through every chunk of entities, the
beyond exit in a late and in the last chunk, the exact length sum where the folded one is blind, a gram bucket
saturated on both sides, one 300-row entity behind 120 tiny ones. Integer equality throughout."""
import numpy as np
import pytest

import po_knn_ref as KR
import po_many_cases as PM
from namazu_amd import _lib
from namazu_amd import historystorage as hs
from test_align_po_gpu import check_projection, same_profile
from test_align_wide_gpu import check
from test_po_many_host import MAP_NAMES, expected, expected_counters, family_counts

pytestmark = pytest.mark.gpu

NONE = _lib.NMZ_NONE
BANDS = (0, 8, 31, 32, 63, 64)


def family_store(name):
    _, trs, ents, G = PM.store(name)
    return hs.TraceSet(list(trs)), np.concatenate(ents), G


def same_lists(got, want, what):
    assert np.array_equal(got[0], want[0]), what
    assert np.array_equal(got[1], want[1]), what


# ---- 1. the projection against numpy ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", MAP_NAMES)
def test_projection_of_the_family(ctx, name):
    ts, ent, G = family_store(name)
    got = check_projection(ctx, ts, ent, G)
    assert len(got.psym) == int((ent != NONE).sum()) < len(ent)
    if name == "dense":  # chunks of 64 elements with dozens of distinct ids: the match-any loop's rounds
        distinct = [len(set(ent[c:c + 64].tolist()) - {NONE}) for c in range(0, 640, 64)]
        assert max(distinct) >= 48


@pytest.mark.parametrize("pattern", ["descending", "one", "cycle65"])
def test_projection_hand_traces(ctx, pattern):
    """1,024 elements with the ids 1023 .. 0: 64 distinct ids in every chunk, 64 rounds of the match-any loop, every
    entity of length 1. 64 elements of one id: one round, the whole wave one group. Ids cycling over 65 values: every
    group straddles a chunk joint, and the counters carry from chunk to chunk."""
    rng = np.random.default_rng(9)
    if pattern == "descending":
        ent, G = np.arange(1023, -1, -1, dtype=np.uint32), 1024
    elif pattern == "one":
        ent, G = np.full(64, 37, np.uint32), 64
    else:
        ent, G = (np.arange(65 * 64 + 7) % 65).astype(np.uint32), 65
    ts = hs.TraceSet([rng.integers(0, 2**63, size=len(ent)).astype(np.uint64)])
    got = check_projection(ctx, ts, ent, G)
    if pattern == "descending":
        assert np.array_equal(got.psrc, np.arange(1023, -1, -1, dtype=np.uint32))
        assert np.array_equal(got.poff, np.arange(1025, dtype=np.uint64))
    elif pattern == "one":
        assert np.array_equal(got.psym, ts.sym[:64]) and got.trace(0, 37)[1].tolist() == list(range(64))


# ---- 2. the scripts, every slot of every pair ------------------------------------------------------------------------
@pytest.mark.parametrize("w", [8, 64, 65, 256])
@pytest.mark.parametrize("name", MAP_NAMES)
def test_scripts(ctx, name, w):
    """All ordered pairs of 18 traces with every variant kind, at the narrow aligner's last band, the wide aligner's
    first and a band that holds the 66 edits of a fold pair; several batches of sub-pairs at 256 under "g1024"."""
    ts, ent, G = family_store(name)
    pairs = PM.ordered_pairs(PM.SAMPLE)
    dist, ops = expected(name, pairs, w)
    print(name, w, "within, not empty", int(((dist > 0) & (dist <= w)).sum()), "beyond", int((dist > w).sum()))
    assert ((dist > 0) & (dist <= w)).sum() >= 16 and (dist > w).sum() >= 16
    es = hs.edit_scripts_po(ts, ent, pairs, w, n_entities=G, ctx=ctx)
    check(es, dist, ops)
    if name == "g1024":  # ops in 8 entities over all four waves of k_po_gather's scan (256 ids each)
        p = pairs.tolist().index([PM.index_of("base"), PM.index_of("spread8")])
        _, _, ents, _ = PM.store(name)
        assert es.dist[p] == 8
        seg = hs.script_by_entity(ents[pairs[p, 0]], ents[pairs[p, 1]], es.ops[p][:8])
        assert len(seg) >= 8 and len({g // 256 for g in seg}) >= 3


def test_scripts_at_the_widest_band(ctx):
    """30 pairs at band 1,024 under "g1024": 12.6 MB of sub-pair ops per pair, two batches of the 256 MiB budget."""
    name, w = "g1024", 1024
    ts, ent, G = family_store(name)
    pairs = PM.ordered_pairs(PM.SAMPLE_WIDEST, with_self=False)
    dist, ops = expected(name, pairs, w)
    assert len(pairs) == 30 and (dist <= w).all() and (dist > 256).sum() >= 8
    check(hs.edit_scripts_po(ts, ent, pairs, w, n_entities=G, ctx=ctx), dist, ops)


# ---- 3. the profile --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", [64, 256])
def test_profile(ctx, w):
    """nmz_ed_diff_profile_po against nmz_move_profile_wide_host over the host PO scripts: the definition."""
    name = "g1024"
    ts, ent, G = family_store(name)
    pairs = PM.ordered_pairs(PM.SAMPLE)
    dist, ops = expected(name, pairs, w)
    want = hs.move_profile_of_wide(ts, pairs, hs.EditScripts(dist, ops, w), host=True)
    got = hs.move_profile_po(ts, ent, pairs, w, n_entities=G, ctx=ctx)
    same_profile(got, want)
    assert int(got.info["n_scripts"]) >= 16 and int(got.info["n_beyond"]) >= 16 and int(got.info["n_ops"]) > 1000


# ---- 4. the search ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", BANDS)
@pytest.mark.parametrize("name", MAP_NAMES)
def test_knn(ctx, name, w):
    """Store = queries = the family: two blocks of candidates. k = 64 of 66 or 67 eligible; q_self = NULL lets each
    trace find itself at 0 first. The counters equal the counts made on the CPU."""
    ts, ent, G = family_store(name)
    n = len(ts)
    Dw = np.minimum(family_counts(name)[0], w + 1)
    index = hs.PoSimilarityIndex(ts, ent, w, ctx=ctx, n_entities=G, max_queries=128, max_query_elems=int(ts.off[-1]))
    try:
        for k in (1, 8, 64):
            for q_self in (np.arange(n, dtype=np.uint32), None):
                got = index.query_csr(ts, ent, k, q_self)
                same_lists(got, KR.knn(Dw, k, q_self), (name, w, k, q_self is None))
                c = index.counters()
                assert c == expected_counters(name, w, self_excluded=q_self is not None), (name, w, k)
        if w >= 8:
            assert c["filtered"] >= 100 and c["length_sum"] >= 16 and c["dp"] - c["in_band"] >= 32
    finally:
        index.close()


@pytest.mark.parametrize("name", MAP_NAMES)
def test_knn_filter_off_and_one_shot(ctx, name):
    w = 32
    ts, ent, G = family_store(name)
    n = len(ts)
    q_self = np.arange(n, dtype=np.uint32)
    Dw = np.minimum(family_counts(name)[0], w + 1)
    lists = {}
    for opts in (0, _lib.NMZ_PO_KNN_OPT_WHOLE_BLOCKS, _lib.NMZ_PO_KNN_OPT_NO_FILTER | _lib.NMZ_PO_KNN_OPT_WHOLE_BLOCKS,
                 _lib.NMZ_PO_KNN_OPT_NO_FILTER):
        index = hs.PoSimilarityIndex(ts, ent, w, ctx=ctx, n_entities=G, max_queries=128,
                                     max_query_elems=int(ts.off[-1]), opts=opts)
        try:
            lists[opts] = index.query_csr(ts, ent, 64, q_self)
            c = index.counters()
            assert c == expected_counters(name, w, no_filter=bool(opts & _lib.NMZ_PO_KNN_OPT_NO_FILTER))
        finally:
            index.close()
    assert c["filtered"] == 0 and c["length_sum"] + c["dp"] == n * (n - 1) and c["length_sum"] >= 100
    for opts in (1, 2, 3):
        assert lists[0][0].tobytes() == lists[opts][0].tobytes() and lists[0][1].tobytes() == lists[opts][1].tobytes()
    same_lists(lists[0], KR.knn(Dw, 64, q_self), name)
    same_lists(hs.po_knn(ts, ent, ts, ent, 8, w, n_entities=G, q_self=q_self, ctx=ctx), KR.knn(Dw, 8, q_self), name)
