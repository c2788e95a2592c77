"""CPU: the host forms of the PO path on the family of tests/po_many_cases.py -- 200 populated entities per trace under
n_entities = 1,024 and 203 -- against the definition, and the counts that keep tests/test_po_many_gpu.py from being
vacuous.

nmz_ed_align_po_host is tied to tests/po_ref.py op for op and nmz_po_knn_bound_host to tests/po_knn_ref.py on a sample
of pairs with every variant kind under both maps; the bound is shown to be a bound on every pair; and the floors on
what the family makes K10 and K11 do -- pairs filtered, settled by the length sum, through the DP and beyond the band
in a late chunk of entities -- are asserted from the host forms and a plain Levenshtein alone. `family_counts` and
`expected_counters` are what the GPU module expects of the kernel's counters. Every comparison is integer equality."""
import functools

import numpy as np
import pytest

import align_ref as AR
import ed_cases as EC
import po_knn_ref as KR
import po_many_cases as PM
import po_ref as PR
from namazu_amd import _lib
from namazu_amd import historystorage as hs
from test_align_po_host import po_slots
from test_po_knn_host import counters_from

NONE = _lib.NMZ_NONE
NONE3 = (NONE,) * 3
MAP_NAMES = ("g1024", "dense")


# ---- the host forms over the family, once ----------------------------------------------------------------------------
_memo = {}


def expected(name, pairs, w):
    """dist[P], ops[P][w] of nmz_ed_align_po_host over the family, computed once per (map, band, pair)."""
    _, trs, ents, G = PM.store(name)
    dist = np.zeros(len(pairs), np.uint32)
    ops = np.zeros((len(pairs), w), _lib.EDIT_OP_DTYPE)
    for p, (i, j) in enumerate(np.asarray(pairs).tolist()):
        key = (name, w, i, j)
        if key not in _memo:
            _memo[key] = po_slots(trs[i], ents[i], trs[j], ents[j], G, w)
        dist[p], ops[p] = _memo[key]
    return dist, ops


@functools.lru_cache(maxsize=None)
def family_bounds(name):
    """LEN[n][n] = LB_len and GRAM[n][n] = LB_gram of nmz_po_knn_bound_host over every ordered pair."""
    _, trs, ents, G = PM.store(name)
    n = len(trs)
    LEN, GRAM = np.zeros((n, n), np.uint64), np.zeros((n, n), np.uint64)
    for i in range(n):
        for j in range(n):
            LEN[i, j], GRAM[i, j] = hs.po_knn_bounds(trs[i], ents[i], trs[j], ents[j], G)
    return LEN, GRAM


@functools.lru_cache(maxsize=None)
def family_counts(name):
    """Over the family under map `name`, the (i, i) pairs included: D[n][n] = the PO distances from the host form (at
    the first of the bands 64, 512 and 1,024 that holds the pair: a distance is the same at every band that holds it,
    and a narrow pass costs a fraction of a wide one; 1,025 beyond them all), LB[n][n] = max(LB_len, LB_gram) from the host form, LS[n][n] = the exact sum of the entities' length
    differences."""
    _, trs, ents, G = PM.store(name)
    n = len(trs)
    D = np.zeros((n, n), np.uint32)
    for i in range(n):
        for j in range(n):
            for w in (64, 512, 1024):
                D[i, j] = po_slots(trs[i], ents[i], trs[j], ents[j], G, w)[0]
                if D[i, j] <= w:
                    break
    per = np.stack([np.bincount(e[e != NONE], minlength=G) for e in ents]).astype(np.int64)
    LS = np.abs(per[:, None, :] - per[None, :, :]).sum(axis=2).astype(np.uint64)
    return D, np.maximum(*family_bounds(name)), LS


def expected_counters(name, w, self_excluded=True, no_filter=False):
    """The kernel's four counters for store = queries = the family at band w, from the host forms alone."""
    return counters_from(*family_counts(name), w, self_excluded=self_excluded, no_filter=no_filter)


# ---- 1. the sample against the definition ----------------------------------------------------------------------------
def sample_pairs():
    """68 ordered pairs: the base against a trace of every variant and back, and the pairs inside each variant kind
    that the kernels' paths are built for."""
    vs_base = ("plain0", "plain7", "chunk0_1", "chunk0_33", "chunk1_5", "chunk7_9", "chunk15_5", "chunk15_33", "spread8",
               "spread9", "spread33", "spread65", "foldbase", "fold3", "fold17", "sat300_0", "sat256_44")
    inner = [("plain3", "plain21"), ("chunk0_5", "chunk1_9"), ("chunk7_33", "chunk15_9"), ("chunk15_1", "chunk15_33"),
             ("spread8", "spread9"), ("spread16", "spread65"), ("spread32", "spread64"), ("chunk15_9", "spread33"),
             ("foldbase", "fold5"), ("foldbase", "fold33"), ("fold3", "fold17"), ("fold5", "fold33"), ("fold10", "fold38"),
             ("sat256_44", "sat260_40"), ("sat290_0", "sat300_0"), ("sat320_0", "sat299_1"), ("fold33", "sat300_0")]
    names = [("base", v) for v in vs_base] + inner
    pairs = [(PM.index_of(a), PM.index_of(b)) for a, b in names]
    pairs += [(j, i) for i, j in pairs]
    kinds = {PM.kind(PM.family()[0][i]) for p in pairs for i in p}
    assert len(set(pairs)) == len(pairs) >= 60 and kinds == set(PM.KINDS)
    return pairs


def test_family_shape():
    names, trs, ents, seqs = PM.family()
    ids = PM.populated()
    assert len(trs) >= 65 and len(ids) == 200 and set(PM.JOINTS) <= set(ids)
    assert sum(PM.kind(n) == "plain" for n in names) >= 20
    for t, e, s in zip(trs, ents, seqs):
        assert 650 <= len(t) <= 1000 and set(e[e != NONE].tolist()) <= set(ids)
        assert 0.02 <= float((e == NONE).mean()) <= 0.04
        proj = PR.project(t.tolist(), e.tolist())
        assert {g: proj[g][0] for g in proj} == {g: EC.encode(s[g]).tolist() for g in ids if s[g]}
    base = seqs[0]
    assert all(1 <= len(base[g]) <= 6 and {x // 4 for x in base[g]} == {g} for g in ids)
    dense = PM.store("dense")
    assert dense[3] == 203 and max(int(e[e != NONE].max()) for e in dense[2]) == 199
    assert PM.to_map("dense", 72) - PM.to_map("dense", 40) == 32 == PM.to_map("dense", 732) - PM.to_map("dense", 700)


@pytest.mark.parametrize("w", [8, 64, 256])
def test_po_host_equals_definition_on_the_sample(w):
    """Distance and every op, sentinels behind them, under both maps; the maps give the same distance and the same
    ops (the rank map keeps the entities' order, and an op holds positions), segment by segment after mapping the ids."""
    pairs = sample_pairs()
    within = beyond = 0
    got = {}
    for name in MAP_NAMES:
        _, trs, ents, G = PM.store(name)
        for i, j in pairs:
            want = PR.script(trs[i].tolist(), ents[i].tolist(), trs[j].tolist(), ents[j].tolist(), w)
            d, ops = po_slots(trs[i], ents[i], trs[j], ents[j], G, w)
            k = d if d <= w else 0
            assert d == want[0] and AR.as_tuples(ops[:k]) == (want[1] or []), (name, w, i, j)
            assert AR.as_tuples(ops[k:]) == [NONE3] * (w - k)
            got[name, i, j] = (d, ops, hs.script_by_entity(ents[i], ents[j], ops[:k]))
            within += 0 < d <= w
            beyond += d > w
    for i, j in pairs:
        a, b = got["g1024", i, j], got["dense", i, j]
        assert a[0] == b[0] and a[1].tobytes() == b[1].tobytes()
        assert [PM.to_map("dense", g) for g in a[2]] == list(b[2])
        assert all(a[2][g].tobytes() == b[2][PM.to_map("dense", g)].tobytes() for g in a[2])
    print(w, "within", within, "beyond", beyond)
    assert within >= 16 and beyond >= (16 if w < 256 else 4)


def test_bound_host_equals_definition_on_the_sample():
    for name in MAP_NAMES:
        _, trs, ents, G = PM.store(name)
        LEN, GRAM = family_bounds(name)
        for i, j in sample_pairs():
            want = KR.bounds(trs[i].tolist(), ents[i].tolist(), trs[j].tolist(), ents[j].tolist())
            assert (int(LEN[i, j]), int(GRAM[i, j])) == want, (name, i, j)


# ---- 2. the bound is a bound, and the family is not vacuous --------------------------------------------------------------
@pytest.mark.parametrize("name", MAP_NAMES)
def test_bound_is_a_bound_and_the_family_is_not_vacuous(name):
    """Over the 4,556 ordered pairs i != j at w = 8 / 32 / 64, "g1024" then "dense": 2,604 / 1,648 / 854 and 2,592 /
    1,662 / 854 filtered, 24 / 42 / 36 and 28 / 40 / 36 settled by the length sum, 1,928 / 2,866 / 3,666 and 1,936 /
    2,854 / 3,666 through the DP, of which 318 / 356 / 210 and 326 / 344 / 210 end beyond the band: 246 / 352 / 208 and
    250 / 332 / 204 of those pass it in a chunk of entities behind the first, 152 / 102 / 118 and 154 / 88 / 82 in the
    last. 62 / 50 / 36 and 64 / 48 / 36 pairs have LB_len <= w < the length sum. 930 pairs i != j are PO-equal."""
    names = PM.family()[0]
    D, LB, LS = family_counts(name)
    LEN = family_bounds(name)[0]
    n = len(D)
    off = ~np.eye(n, dtype=bool)
    assert not (LB > D).any() and not (LS > D).any() and not D[~off].any()
    n_chunks = (PM.MAPS[name] + 63) // 64
    for w in (8, 32, 64):
        c = expected_counters(name, w)
        filt = off & (LB > w)
        dp_beyond = off & ~filt & (LS <= w) & (D > w)
        blind = int((off & (LEN <= w) & (LS > w)).sum())
        chunks = [PM.passing_chunk(name, i, j, w) for i, j in np.argwhere(dp_beyond).tolist()]
        assert None not in chunks
        late, last = sum(ch >= 1 for ch in chunks), sum(ch == n_chunks - 1 for ch in chunks)
        print(name, w, c, "DP beyond", len(chunks), "LB_len <= w < length sum", blind, "passing in a chunk >= 1", late,
              "in the last chunk", last)
        assert c["filtered"] == int(filt.sum()) >= 100 and c["length_sum"] >= 16 and c["dp"] >= 100
        assert c["dp"] - c["in_band"] == len(chunks) >= 32
        assert blind >= 16 and late >= 16 and last >= 8
    assert int((off & (D == 0)).sum()) >= 40
    _, trs, ents, _ = PM.store(name)
    sat = [i for i, nm in enumerate(names) if PM.kind(nm) == "sat"]
    assert len(sat) == len(PM.SAT)
    for i in sat:  # one bucket at 255 where entity 700 holds 256 elements or more
        gram = KR.profile(trs[i].tolist(), ents[i].tolist())[1]
        assert (max(gram) == 255) == (names[i] != "sat200_100") and (gram.count(255) == 1) == (names[i] != "sat200_100")
    # 199 grams against 299 counted as 255, 99 and 1 against none: ceil(156 / 4) = 39, less where a bucket is shared;
    # the filter settles the pair at 32 only because the count stops at 255 and not below (25 at 127)
    i, j = PM.index_of("sat200_100"), PM.index_of("sat300_0")
    assert (int(LEN[i, j]), int(LS[i, j])) == (0, 200) and 32 < int(LB[i, j]) <= 39
    assert any(8 <= D[i, j] <= 32 for i in sat for j in sat)


def test_both_maps_give_the_same_distances():
    assert np.array_equal(family_counts("g1024")[0], family_counts("dense")[0])
    assert np.array_equal(family_counts("g1024")[2], family_counts("dense")[2])
    # 40 = 72 and 700 = 732 (mod 32) under both maps: the folded bound is blind where the fold and sat variants differ
    for name in MAP_NAMES:
        LEN, LS = family_bounds(name)[0], family_counts(name)[2]
        i, j = PM.index_of("foldbase"), PM.index_of("fold33")
        assert (LEN[i, j], LS[i, j]) == (0, 66)
        i, j = PM.index_of("sat300_0"), PM.index_of("sat256_44")
        assert (LEN[i, j], LS[i, j]) == (0, 88)


def test_the_sample_of_the_script_tests_is_not_vacuous():
    """tests/test_po_many_gpu.py's pairs: at every band up to 256 at least 16 scripts in band and not empty and 16
    beyond; an in-band script with ops in at least 8 entities over at least 3 of k_po_gather's waves (256 ids each)."""
    pairs = PM.ordered_pairs(PM.SAMPLE)
    assert len(pairs) == 18 * 18 and {PM.kind(n) for n in PM.SAMPLE} == set(PM.KINDS)
    for name in MAP_NAMES:
        for w in (8, 64, 65, 256):
            dist, _ = expected(name, pairs, w)
            print(name, w, "within", int(((dist > 0) & (dist <= w)).sum()), "beyond", int((dist > w).sum()))
            assert ((dist > 0) & (dist <= w)).sum() >= 16 and (dist > w).sum() >= 16
    assert wide_script_entities(8) >= (8, 3)
    assert len(PM.ordered_pairs(PM.SAMPLE_WIDEST, with_self=False)) == 30


def wide_script_entities(w):
    """(entities, waves of k_po_gather) that the host script of base -> spread8 under "g1024" has ops in."""
    _, trs, ents, G = PM.store("g1024")
    i, j = PM.index_of("base"), PM.index_of("spread8")
    d, ops = expected("g1024", [(i, j)], w)
    assert d[0] == 8 <= w
    seg = hs.script_by_entity(ents[i], ents[j], ops[0][:8])
    return len(seg), len({g // 256 for g in seg})
