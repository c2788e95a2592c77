"""The wide PO k-NN search's second family and its expected counters (not a test module).

Over the 42-trace family of tests/test_po_knn_host.py almost no pair passes both filters and then ends beyond a wide
band, so that family alone would leave k_po_knn_wide's budget cut-off untested. The family here ("cut") is made for
it: 28 seeded traces over five entities whose lengths stay (almost) the same between traces, so that only the gram
bound can filter, and whose distances spread over every band from 65 to 1,024.

  base      five entities with sequences of 40, 200, 330, 500 and 1,900 symbols over one 4-letter alphabet (the
            symbols do not tell the entity), randomly interleaved: at band 1,024 their clamped bands fall on 1, 2, 3,
            5 and 9 cells per thread;
  0 .. 15   for every subset of the entities 0, 1, 2 and 4, the sequences of that subset replaced with fresh random
            ones;
  16 .. 21  one entity's sequence rotated: the PO distance is about twice the shift while the lengths stay;
  22 .. 27  the last entity shortened by 50 .. 600 and one earlier entity replaced, so the last entity's length check
            meets a budget that the earlier entities have used.

Everything expected comes from the host forms alone: D from nmz_ed_align_po_host at band 1,024, the bounds from
nmz_po_knn_bound_host, the per-entity Lev_g from nmz_ed_align_wide_host over the projections (the host form with one
entity), and the kernel's nine counters from the walk DESIGN.md section 4 "K11w" describes."""
import functools

import numpy as np

import po_knn_ref as KR
from namazu_amd import historystorage as hs
from test_align_po_host import gpu_family, po_slots
from test_align_wide_host import wide_slots
from test_po_knn_host import family_counts

BANDS = (65, 127, 128, 255, 256, 383, 384, 639, 640, 1024)
TOP = 1024  # one host pass at the widest band gives min(d, w + 1) for every w
LENS = (40, 200, 330, 500, 1900)
REPLACED = (0, 1, 2, 4)  # the entities whose subsets the first 16 variants replace
ALPHABET = np.array([11, 22, 33, 44], np.uint64)
ROTATIONS = ((4, 20), (4, 45), (4, 70), (4, 100), (4, 300), (3, 60))
CUTS = ((50, 0), (100, 1), (200, 0), (300, 1), (450, 2), (600, 1))  # (symbols cut from entity 4, entity replaced)
STEP_CELLS = (1, 2, 3, 5, 9)


def cells(w):
    """Cells per thread for a band: 2 w + 1 <= 256 C over C = 1, 2, 3, 5, 9."""
    for c, top in zip(STEP_CELLS, (127, 255, 383, 639)):
        if w <= top:
            return c
    return 9


def _interleave(rng, seqs):
    order = rng.permutation(np.repeat(np.arange(len(seqs)), [len(s) for s in seqs]))
    at = [0] * len(seqs)
    sym = np.zeros(len(order), np.uint64)
    for p, g in enumerate(order.tolist()):
        sym[p] = seqs[g][at[g]]
        at[g] += 1
    return sym, order.astype(np.uint32)


@functools.lru_cache(maxsize=None)
def cut_family():
    """(traces, entities, n_entities) of the "cut" family."""
    rng = np.random.default_rng(20240611)
    fresh = lambda L: ALPHABET[rng.integers(0, 4, size=L)]
    base = [fresh(L) for L in LENS]
    out = []
    for subset in range(16):
        out.append(_interleave(rng, [fresh(L) if g in REPLACED and subset >> REPLACED.index(g) & 1 else base[g]
                                     for g, L in enumerate(LENS)]))
    for g, shift in ROTATIONS:
        seqs = list(base)
        seqs[g] = np.roll(base[g], shift)
        out.append(_interleave(rng, seqs))
    for cut, g in CUTS:
        seqs = list(base)
        seqs[g] = fresh(LENS[g])
        seqs[4] = base[4][:LENS[4] - cut]
        out.append(_interleave(rng, seqs))
    return tuple(t for t, _ in out), tuple(e for _, e in out), len(LENS)


def family(key):
    """(traces, entities, n_entities): "cut" or the 42-trace family under the map "mod2" / "sparse"."""
    return cut_family() if key == "cut" else gpu_family(key)


@functools.lru_cache(maxsize=None)
def matrices(key):
    """D[n][n] (the PO distance from one band-1,024 host pass, 1,025 beyond it), LB[n][n] = max(LB_len, LB_gram),
    LS[n][n] = the exact length sum, then per populated entity (ascending ids) LEV[n][n][E] = Lev_g capped at 1,025
    and LEN[n][E] = the projection's length."""
    trs, ents, G = family(key)
    n = len(trs)
    ids = sorted({int(g) for e in ents for g in np.unique(e).tolist() if g != KR.NONE})
    proj = [[np.ascontiguousarray(t[e == g]) for g in ids] for t, e in zip(trs, ents)]
    LEN = np.array([[len(p) for p in row] for row in proj], np.int64)
    LEV = np.zeros((n, n, len(ids)), np.int64)
    for i in range(n):
        for j in range(i + 1, n):  # Lev is symmetric
            for x in range(len(ids)):
                LEV[i, j, x] = LEV[j, i, x] = wide_slots(proj[i][x], proj[j][x], TOP)[0]
    if key == "cut":
        D = np.zeros((n, n), np.uint32)
        LB = np.zeros((n, n), np.uint64)
        LS = np.zeros((n, n), np.uint64)
        for i in range(n):
            for j in range(n):
                if i < j:
                    D[i, j] = D[j, i] = po_slots(trs[i], ents[i], trs[j], ents[j], G, TOP)[0]
                if i != j:
                    LB[i, j] = max(hs.po_knn_bounds(trs[i], ents[i], trs[j], ents[j], G))
                    LS[i, j] = KR.length_sum(ents[i], ents[j])
        for i, j in ((1, 0), (17, 3), (27, 22), (9, 25)):  # the host distance is symmetric: four pairs the other way
            assert po_slots(trs[i], ents[i], trs[j], ents[j], G, TOP)[0] == D[i, j]
    else:
        D, LB, LS = family_counts(key)
    # the per-entity distances add up to the PO distance wherever that is within the pass's band
    assert np.array_equal(np.minimum(LEV.sum(axis=2), TOP + 1), D.astype(np.int64))
    return D, LB, LS, LEV, LEN


def walk(key, i, j, w, full_band=False):
    """The kernel's walk over one pair that reached the DP at band w: (steps per C [5], how it ended), the end one of
    "in" (within the band), "length" (an entity's length difference exceeded the budget) or "dp" (an entity's
    distance did)."""
    _, _, _, LEV, LEN = matrices(key)
    steps = [0] * 5
    total = 0
    for x in range(LEN.shape[1]):
        n, m = int(LEN[i, x]), int(LEN[j, x])
        if n == 0 and m == 0:
            continue
        r = w - total
        if abs(n - m) > r:
            return steps, "length"
        steps[STEP_CELLS.index(cells(w) if full_band else cells(min(r, max(n, m))))] += 1
        if LEV[i, j, x] > r:
            return steps, "dp"
        total += int(LEV[i, j, x])
    return steps, "in"


def pair_classes(key, w, self_excluded=True, no_filter=False):
    """Boolean matrices over the ordered pairs at band w: eligible, filtered, settled by the length sum, ran a DP."""
    D, LB, LS, _, _ = matrices(key)
    elig = ~np.eye(len(D), dtype=bool) if self_excluded else np.ones(D.shape, bool)
    filt = elig & (LB > w) & (not no_filter)
    lens = elig & ~filt & (LS > w)
    return elig, filt, lens, elig & ~filt & ~lens


@functools.lru_cache(maxsize=None)
def expected_counters(key, w, self_excluded=True, no_filter=False, full_band=False):
    """The nine counters of a search with store = queries = the family at band w (PoSimilarityIndex.counters' names),
    from the host forms alone (computed once per case: do not change the dict). A band <= 64 runs the narrow kernel: no
    entity step is counted."""
    D = matrices(key)[0]
    elig, filt, lens, dp = pair_classes(key, w, self_excluded, no_filter)
    steps = np.zeros(5, np.int64)
    if w > 64:
        for i, j in np.argwhere(dp).tolist():
            s, end = walk(key, i, j, w, full_band)
            assert (end == "in") == (D[i, j] <= w)
            steps += s
    out = {"filtered": int(filt.sum()), "length_sum": int(lens.sum()), "dp": int(dp.sum()),
           "in_band": int((elig & (D <= w)).sum())}
    out.update(zip(hs.PoSimilarityIndex.STEP_NAMES, (int(v) for v in steps)))
    return out


def store(key):
    """(TraceSet, entity[N], n_entities) of a family."""
    trs, ents, G = family(key)
    return hs.TraceSet(list(trs)), np.concatenate(ents), G
