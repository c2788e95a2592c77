"""Restatement of the trace signature and its classes for the tests (not a test module).

A trace is the multiset {(symbol, rank)}: rank = the position (exact mode) or the running count of the element's
entity (partial-order mode); an element is skipped when its entity is NMZ_NONE or, when a bound is given, >= bound
(include/nmz_gpu.h). The signature sums two 64-bit mixes of every pair mod 2^64 and adds the count terms; the
formulas are those of csrc/sig_dev.h (fmix64, rank_key_a / rank_key_b, mix2k, sig_final_lo / sig_final_hi), written
here on plain Python integers masked to 64 bits: no numpy arithmetic, so no silent wrap to trust, and nothing shared
with the kernel (one element at a time, a dict of counters; no steps, batches, ballots or key table).
tests/delivery_ref.py keeps the independent numpy form."""

M64 = (1 << 64) - 1
M32 = (1 << 32) - 1
NONE = 0xFFFFFFFF
INT64_MAX = (1 << 63) - 1


def fmix64(x):
    x &= M64
    x ^= x >> 33
    x = (x * 0xff51afd7ed558ccd) & M64
    x ^= x >> 33
    x = (x * 0xc4ceb9fe1a85ec53) & M64
    x ^= x >> 33
    return x


def rank_key_a(r):
    return fmix64((r + 0x9e3779b97f4a7c15) & M64)


def rank_key_b(r):
    return fmix64((((r << 32) | ((r ^ 0x5bd1e995) & M32)) + 0x632be59bd9b4e019) & M64)


_keys = {}  # rank -> (ka, kb), every entry from the two formulas above (a cache, no table bound)


def rank_keys(r):
    k = _keys.get(r)
    if k is None:
        k = _keys[r] = (rank_key_a(r), rank_key_b(r))
    return k


def mix2k(s, ka, kb):
    """The two summands of a symbol under a rank's two keys."""
    t = fmix64(s ^ ka)
    u = ((t ^ kb) * 0x94d049bb133111eb) & M64
    return t, u ^ (u >> 29)


def _ints(a):
    return a.tolist() if hasattr(a, "tolist") else [int(x) for x in a]


def ranks(n, entity=None, bound=None):
    """rank per element, None for a skipped one."""
    if entity is None:
        return list(range(n))
    count, out = {}, []
    for e in _ints(entity):
        if e == NONE or (bound is not None and e >= bound):
            out.append(None)
        else:
            r = count.get(e, 0)
            count[e] = r + 1
            out.append(r)
    return out


def signature(sym, entity=None, bound=None):
    """(lo, hi) of one trace: sym[n] uint64 symbols, entity[n] ids or None (exact mode)."""
    sym = _ints(sym)
    acc1 = acc2 = counted = 0
    for s, r in zip(sym, ranks(len(sym), entity, bound)):
        if r is None:
            continue
        assert 0 <= s <= M64 and 0 <= r <= M32
        a, b = mix2k(s, *rank_keys(r))
        acc1 = (acc1 + a) & M64
        acc2 = (acc2 + b) & M64
        counted += 1
    return (acc1 + fmix64(counted + 1)) & M64, acc2 ^ fmix64((counted << 1) | 1)


def first_equal(sigs):
    """first_equal[i] = the smallest j with sigs[j] == sigs[i]."""
    seen = {}
    return [seen.setdefault((int(lo), int(hi)), i) for i, (lo, hi) in enumerate(sigs)]


def class_rep(first_equal, gaps):
    """At a class head h: the member with the largest min_gap_ns, ties to the smallest index; NMZ_NONE elsewhere."""
    rep = [NONE] * len(first_equal)
    for i, h in enumerate(first_equal):
        if rep[h] == NONE or int(gaps[i]) > int(gaps[rep[h]]):
            rep[h] = i
    return rep


def n_classes(first_equal):
    return sum(1 for i, h in enumerate(first_equal) if h == i)
