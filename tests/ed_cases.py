"""Structured trace families for the edit-distance tests (not a test module).

The generators of tests/test_ed_gpu.py and namazu_amd/synth.py give pairs whose best alignment is the main diagonal
plus a tail. The families here put the optimal path away from the band's centre: indels at the start (the path runs
on diagonal +-d, d = w rides the band edge), shifts, rotations (same bigram profile as the base, so the q-gram
bound must let them through), an offset held over one block only, random edits, and periodic traces (dense match
bitmaps, all-ones propagate words).

Everything a test compares with comes from the CPU oracle: `reference(case)` holds the ordered-pair distance
matrix, `knn_from(D, order, k)` turns it into the all-pairs k-NN lists of any store order, and `stats(case)` counts
what the family exercises (tests/test_ed_offdiag.py asserts those counts, so the GPU comparison cannot pass
vacuously)."""
import functools
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from oracle import oracle as O

GOLDEN = np.uint64(0x9E3779B97F4A7C15)
N_FRESH = 4  # F_d draws from this many symbols, none of them in the base's alphabet


def encode(ids):
    """Dense symbol ids -> u64 event hashes."""
    return np.asarray(ids, np.int64).astype(np.uint64) * GOLDEN + np.uint64(5)


def shifts_for(w, unit=32):
    """{1, w/2, w-1, w, w+1} plus d = 0, +-1 mod `unit` at the first and the last multiple of `unit` up to w + 1:
    the working diagonal on the joints of the layout (unit = 32 for the bit-parallel kernels' words, 32 * KL for
    the wide kernel's lanes)."""
    ds = {1, w // 2, w - 1, w, w + 1}
    mult = list(range(unit, w + 2, unit))
    for m in mult[:1] + mult[-1:]:
        ds |= {m - 1, m, m + 1}
    return sorted(d for d in ds if 1 <= d <= w + 1)


def _edited(a, n_edits, alphabet, rng):
    t = list(a)
    for _ in range(n_edits):
        op, p = int(rng.integers(0, 3)), int(rng.integers(0, max(len(t), 1)))
        if op == 0:
            t.insert(p, int(rng.integers(0, alphabet)))
        elif op == 1 and len(t) > 1:
            del t[p]
        elif t:
            t[p] = int(rng.integers(0, alphabet))
    return np.array(t, np.int64)


def named_family(L, alphabet, w, rng, shifts=None, unit=32, distinct=False):
    """[(name, u64 trace)] over one random base `a` of length L. F_d = d fresh symbols. `shifts` replaces the
    d values derived from w (for bands far beyond the traces' length). `distinct` draws the base without
    replacement (every trace then holds about L distinct symbols, which keeps a large-alphabet store off the
    bit-parallel kernels' compact tables)."""
    a = (rng.choice(alphabet, L, replace=False) if distinct else rng.integers(0, alphabet, size=L)).astype(np.int64)

    def F(d):
        return rng.integers(alphabet, alphabet + N_FRESH, size=d).astype(np.int64)

    cat = np.concatenate
    if shifts is None:
        D = shifts_for(w, unit)
        S = sorted({1, w // 2, w // 2 + 1})
        edits = sorted({1, max(w // 2, 1), w, w + 1})
    else:
        D = S = edits = sorted(shifts)
    D = [d for d in D if d < L]
    S = [d for d in S if 1 <= d < L]
    p = L // 3
    X = sorted({max(1, min(S[len(S) // 2], p - 1) // 2), max(1, min(S[len(S) // 2], p - 1))})
    out = [("a", a)]
    out += [(f"F{d}+a", cat([F(d), a])) for d in D]
    out += [(f"a[{d}:]", a[d:]) for d in D]
    out += [(f"a+F{d}", cat([a, F(d)])) for d in D]
    out += [(f"shift{d}", cat([a[d:], F(d)])) for d in S]
    out += [(f"rot{d}", cat([a[d:], a[:d]])) for d in S]
    out += [(f"block{d}", cat([a[:p], a[p + d:2 * p], F(d), a[2 * p:]])) for d in X]
    out += [(f"edit{e}", _edited(a, e, alphabet, rng)) for e in edits]
    return [(name, encode(t)) for name, t in out]


def family(L, alphabet, w, rng, shifts=None, unit=32, distinct=False):
    return [t for _, t in named_family(L, alphabet, w, rng, shifts, unit, distinct)]


def trimmed_family(L, alphabet, w, rng, n_max, unit=32):
    """At most n_max members for the bands whose oracle is slow, the band-edge members first: a, F_{w-1}/F_w/
    F_{w+1} + a, a[w:], both shifts, the rotation and the offset block, then a[1:] (band edge against
    F_{w-1} + a) and further start indels."""
    fam = dict(named_family(L, alphabet, w, rng, None, unit))
    h = w // 2
    want = ["a", f"F{w - 1}+a", f"F{w}+a", f"F{w + 1}+a", f"a[{w}:]", f"shift{h}", f"shift{h + 1}", f"rot{h}",
            [n for n in fam if n.startswith("block")][-1], "a[1:]", "F1+a", f"a[{w - 1}:]", f"F{h}+a", f"a[{h}:]"]
    return [fam[n] for n in want[:n_max]]


def periodic(w):
    """Tilings over 2-3 symbols at length L = 3w + 7, and constant traces of length L, L - w and L + 1."""
    L = 3 * w + 7

    def tile(pat, n=L):
        return np.resize(np.array(pat, np.int64), n)

    out = [tile([1, 2]), tile([2, 1]), tile([1, 2, 3]), tile([3, 1, 2]), tile([2, 3, 1]), tile([1, 1, 2]),
           tile([1, 2, 1]), tile([1]), tile([1], L - w), tile([1], L + 1)]
    return [encode(t) for t in out]


# ---- the cases of tests/test_ed_offdiag*.py: name -> (plan kind, band, builder) --------------------------------------
def _fam(L, alphabet, w, seed, **kw):
    return lambda: family(L, alphabet, w, np.random.default_rng(seed), **kw)


def _trim(L, alphabet, w, seed, n_max, unit):
    return lambda: trimmed_family(L, alphabet, w, np.random.default_rng(seed), n_max, unit)


def _three(L, alphabet, w, seed, **kw):
    return lambda: sum((family(L, alphabet, w, np.random.default_rng(seed + s), **kw) for s in range(3)), [])


CASES = {
    # bit-parallel (kind 2): template W = 8, 16, 32, 64, then run-time w below W
    "bv-w8": (2, 8, _fam(70, 6, 8, 108)),
    "bv-w16": (2, 16, _fam(130, 20, 16, 116)),
    "bv-w32": (2, 32, _fam(200, 12, 32, 132)),
    "bv-w64": (2, 64, _fam(300, 16, 64, 164)),
    "bv-w5": (2, 5, _fam(100, 4, 5, 105)),
    "bv-w33": (2, 33, _fam(200, 12, 33, 133)),
    "bv-w50": (2, 50, _fam(260, 12, 50, 150)),
    "bv-per8": (2, 8, lambda: periodic(8)),
    "bv-per32": (2, 32, lambda: periodic(32)),
    "bv-per64": (2, 64, lambda: periodic(64)),
    "bv-3fam": (2, 32, _three(200, 12, 32, 900)),  # >= 65 traces: pairs cross a 64-query block
    # tile (kind 1): three families in one store. One base's family holds ~300 distinct symbols, which fit the
    # bit-parallel kernels' direct tables; three bases pass those (> 606 symbols at this length), and bases
    # without repeats keep a query pair's own symbols (>= 600) beyond the compact tables
    "tile-w8": (1, 8, _three(300, 3000, 8, 208, distinct=True)),
    "tile-w16": (1, 16, _three(300, 3000, 16, 216, distinct=True)),
    "tile-w32": (1, 32, _three(300, 3000, 32, 232, distinct=True)),
    # wide (kind 3): a lane holds KL = W / 1024 words
    "wide-w100": (3, 100, _fam(700, 16, 100, 300, unit=32)),
    "wide-w1024": (3, 1024, _fam(1500, 16, 1024, 301, unit=32)),
    "wide-w2048": (3, 2048, _fam(2700, 20, 2048, 302, unit=64)),
    "wide-w4096": (3, 4096, _trim(5000, 30, 4096, 304, 14, 128)),
    "wide-w8192": (3, 8192, _trim(9000, 64, 8192, 308, 10, 256)),
    "wide-per1024": (3, 1024, lambda: periodic(1024)),
    # generic (kind 0): a band beyond the wide kernels
    "generic-w9000": (0, 9000, _fam(120, 12, 9000, 400, shifts=(1, 5, 20))),
}
FEW_FAR = {n for n in CASES if "per" in n} | {"generic-w9000"}  # few pairs beyond the band, by nature
FAMILIES = {"bv-3fam": 3, "tile-w8": 3, "tile-w16": 3, "tile-w32": 3}  # stores of several equal-sized families


def kind(name):
    return CASES[name][0]


def band(name):
    return CASES[name][1]


@functools.lru_cache(maxsize=None)
def traces(name):
    return tuple(CASES[name][2]())


def csr(trs):
    """(off, sym) as the oracle and the library take them."""
    off = np.zeros(len(trs) + 1, np.uint64)
    off[1:] = np.cumsum([len(t) for t in trs])
    sym = np.concatenate(list(trs)) if off[-1] else np.zeros(1, np.uint64)
    return off, np.ascontiguousarray(sym, np.uint64)


def all_ordered_pairs(n):
    i, j = np.divmod(np.arange(n * n, dtype=np.uint32), np.uint32(n))
    return np.stack([i, j], 1).astype(np.uint32)


@functools.lru_cache(maxsize=None)
def reference(name):
    """The oracle's ED_w of every ordered pair, [n, n] (read-only; computed once per process). Bands from 2,048
    (seconds of oracle time) compute i < j only and mirror it; tests/test_ed_offdiag.py checks on the other cases
    that the oracle's matrix is symmetric."""
    trs = traces(name)
    n = len(trs)
    off, sym = csr(trs)
    pairs = all_ordered_pairs(n)
    if band(name) >= 2048 and kind(name) == 3:
        up = pairs[pairs[:, 0] < pairs[:, 1]]
        D = np.zeros((n, n), np.uint32)
        O.lib()
        # one pair per call on 16 Python threads (ctypes drops the GIL): the oracle hands its OpenMP threads
        # chunks of 16 pairs, which would leave these few, long pairs to 3 threads
        with ThreadPoolExecutor(16) as ex:
            d = list(ex.map(lambda pr: int(O.ed_pairs(off, sym, pr[None, :], band(name), nthreads=1)[0]), up))
        D[up[:, 0], up[:, 1]] = d
        D = D + D.T
    else:
        D = O.ed_pairs(off, sym, pairs, band(name), nthreads=16).reshape(n, n)
    D.setflags(write=False)
    return D


def knn_from(D, order, k):
    """The all-pairs k-NN lists (ids, dists) of the store [traces[i] for i in order], from the ordered-pair
    matrix D of the family as built: per query the others by (distance asc, store id asc)."""
    order = np.asarray(order)
    n = len(order)
    Ds = D[np.ix_(order, order)]
    ids = np.zeros((n, k), np.uint32)
    ds = np.zeros((n, k), np.uint32)
    for q in range(n):
        c = np.array([j for j in range(n) if j != q])
        sel = c[np.lexsort((c, Ds[q, c]))][:k]
        ids[q], ds[q] = sel, Ds[q, sel]
    return ids, ds


def diagonal_cost(a, b):
    """Hamming distance over the common prefix + the length difference: what a kernel that never left the main
    diagonal would answer."""
    c = min(len(a), len(b))
    return int((a[:c] != b[:c]).sum()) + abs(len(a) - len(b))


@functools.lru_cache(maxsize=None)
def stats(name):
    """Counts over the ordered pairs (i != j) of a case, from the oracle alone. In a store of several families
    "pairs", "in_band" and "far_in_length_band" count the pairs inside one family (pairs across families are all
    beyond the band: they would only dilute the fractions the conditions are about); the other counts take every
    pair."""
    trs, D, w = traces(name), reference(name), band(name)
    n = len(trs)
    fam = np.arange(n) // (n // FAMILIES.get(name, 1))
    same = fam[:, None] == fam[None, :]
    ln = np.array([len(t) for t in trs], np.int64)
    diff = ln[:, None] - ln[None, :]
    diag = np.array([[diagonal_cost(trs[i], trs[j]) for j in range(n)] for i in range(n)], np.int64)
    off_d = ~np.eye(n, dtype=bool)
    inb = off_d & (D <= w)
    pos = inb & (D > 0)
    return {
        "traces": n,
        "pairs": int((off_d & same).sum()),
        "in_band": int((inb & same).sum()),
        "far_in_length_band": int((off_d & same & (D > w) & (np.abs(diff) <= w)).sum()),
        "in_band_across_families": int((inb & ~same).sum()),
        "in_band_pos": int(pos.sum()),
        "off_diagonal": int((pos & (D < diag)).sum()),
        "half_diagonal": int((pos & (2 * D.astype(np.int64) <= diag)).sum()),
        "edge_longer_query": int((inb & (diff == w)).sum()),
        "edge_longer_candidate": int((inb & (diff == -w)).sum()),
    }
