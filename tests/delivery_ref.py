"""Restatement of the delivery sweep's definition for the tests (not a test module).

Delays come from the C oracle (oracle.replayable_sweep with every seed dumped); the definition of include/nmz_gpu.h
is then applied in numpy on 64-bit integers:

    release[s][e] = arrival_ns[e] + delay[s][e]
    order pi_s    = the counted events by (release asc, event index asc)        (a stable sort of the releases)
    rank          = position in pi_s (exact) or inside the entity's projection of pi_s (PO)
    sig           = sum of mix(sym, rank) + the count terms, the formulas of csrc/sig_dev.h restated here
    gap           = release difference of neighbours of a compared sequence; min_gap_ns, gap_event

and seeds are classed by the symbol sequences the reference compares (visualize.go:51-136): the whole delivered
sequence (exact) or every entity's (PO). Everything is integer: tests compare with equality."""
import numpy as np

from oracle import oracle as O

MS = 1_000_000
NONE = 0xFFFFFFFF
INT64_MAX = 2**63 - 1
STATS_DTYPE = np.dtype([("sig_lo", "<u8"), ("sig_hi", "<u8"), ("min_gap_ns", "<i8"), ("gap_event", "<u4"),
                        ("n_counted", "<u4")])
U = np.uint64


def fmix64(x):
    x = np.atleast_1d(np.asarray(x, U)).copy()
    x ^= x >> U(33)
    x *= U(0xff51afd7ed558ccd)
    x ^= x >> U(33)
    x *= U(0xc4ceb9fe1a85ec53)
    x ^= x >> U(33)
    return x


def rank_keys(r):
    r = np.asarray(r, U)
    ka = fmix64(r + U(0x9e3779b97f4a7c15))
    kb = fmix64(((r << U(32)) | (r ^ U(0x5bd1e995))) + U(0x632be59bd9b4e019))
    return ka, kb


def mix2(sym, rank):
    """The two summands of the pair (symbol, rank)."""
    ka, kb = rank_keys(rank)
    t = fmix64(np.asarray(sym, U) ^ ka)
    u = (t ^ kb) * U(0x94d049bb133111eb)
    return t, u ^ (u >> U(29))


def decimal_seeds(lo, n):
    return [str((lo + i) % 2**64) for i in range(n)]


def delays(seeds, hints, m):
    """delay[s][e] for every seed and hint, from the C oracle's sweep dump."""
    so, sb = O.to_csr(list(seeds))
    ho, hb = O.to_csr(list(hints))
    if not len(seeds):
        return np.zeros((0, len(hints)), np.int64)
    return O.replayable_sweep(so, sb, ho, hb, m, n_dump=len(seeds))[1]


class Ref:
    """stats[S], order[S][G] (event indices in delivery order), release[S][E] and canon[S] (the bytes of the
    compared symbol sequences: equal bytes <=> the reference calls the traces equal)."""

    def __init__(self, dl, arrival, sym, entity=None):
        arrival = np.asarray(arrival, np.int64)
        sym = np.asarray(sym, U)
        S, E = dl.shape
        self.release = arrival[None, :] + dl
        ent = None if entity is None else np.asarray(entity, np.uint32)
        counted = np.arange(E) if ent is None else np.nonzero(ent != NONE)[0]
        G = len(counted)
        # a stable sort of the releases of the counted events, which are in index order: ties go by index
        self.order = counted[np.argsort(self.release[:, counted], axis=1, kind="stable")] if G else \
            np.zeros((S, 0), np.int64)
        groups = [counted] if ent is None else [counted[ent[counted] == v] for v in np.unique(ent[counted])]
        acc1, acc2 = np.zeros(S, U), np.zeros(S, U)
        gap = np.full(S, INT64_MAX, np.int64)
        gev = np.full(S, NONE, np.int64)
        canon = []
        for g in groups:
            rel = self.release[:, g]
            o = np.argsort(rel, axis=1, kind="stable")
            ev = g[o]                                     # [S][n] the entity's events in delivery order
            canon.append(sym[ev])
            a, b = mix2(sym[ev], np.arange(len(g), dtype=U)[None, :])
            acc1 += a.sum(axis=1, dtype=U)
            acc2 += b.sum(axis=1, dtype=U)
            if len(g) > 1:
                d = np.diff(np.take_along_axis(rel, o, axis=1), axis=1)
                mn = d.min(axis=1)
                later = np.where(d == mn[:, None], ev[:, 1:], NONE).min(axis=1)  # smallest later event attaining it
                better = (mn < gap) | ((mn == gap) & (later < gev))
                gap = np.where(better, mn, gap)
                gev = np.where(better, later, gev)
        self.stats = np.zeros(S, STATS_DTYPE)
        self.stats["sig_lo"] = acc1 + fmix64(U(G + 1))
        self.stats["sig_hi"] = acc2 ^ fmix64(U((G << 1) | 1))
        self.stats["min_gap_ns"] = gap
        self.stats["gap_event"] = gev
        self.stats["n_counted"] = G
        cn = np.hstack(canon) if canon else np.zeros((S, 0), U)
        self.canon = [cn[s].tobytes() for s in range(S)]
        self.entity = ent
        self.sym = sym

    def first_equal(self):
        seen, out = {}, np.zeros(len(self.canon), np.uint32)
        for i, c in enumerate(self.canon):
            out[i] = seen.setdefault(c, i)
        return out

    def class_rep(self):
        """At a class head: the member with the largest min_gap_ns, ties to the smallest index; NONE elsewhere."""
        fe = self.first_equal()
        rep = np.full(len(fe), NONE, np.uint32)
        gaps = self.stats["min_gap_ns"]
        for i, h in enumerate(fe):
            if rep[h] == NONE or gaps[i] > gaps[rep[h]]:
                rep[h] = i
        return rep

    def traces(self):
        """The delivered traces as nmz_trace_signatures / nmz_unique_traces take them: (off, sym, entity or None)."""
        S, G = self.order.shape
        off = np.arange(S + 1, dtype=np.uint64) * np.uint64(G)
        sy = np.ascontiguousarray(self.sym[self.order].reshape(-1)) if G else np.zeros(1, U)
        en = None
        if self.entity is not None:
            en = np.ascontiguousarray(self.entity[self.order].reshape(-1)) if G else np.zeros(1, np.uint32)
        return off, sy, en


def class_sizes(first_equal):
    return np.bincount(first_equal, minlength=len(first_equal))


def assert_partition_mixed(first_equal, singletons=True):
    """The condition every class test states first: the reference's partition merges and does not merge."""
    sizes = class_sizes(first_equal)
    assert (sizes >= 2).sum() >= 8, "degenerate input: fewer than 8 classes with >= 2 members"
    if singletons:
        assert (sizes == 1).sum() >= 8, "degenerate input: fewer than 8 singleton classes"


def host_delivery(seeds, hints, arrival, sym, entity, m):
    """nmz_replayable_delivery_host per seed string: (stats[S], order[S][E], release[S][E])."""
    from namazu_amd import _lib
    L = _lib.load()
    ho, hb = O.to_csr(list(hints))
    E = len(hints)
    arr = np.ascontiguousarray(arrival, np.int64)
    sy = np.ascontiguousarray(sym, np.uint64)
    en = None if entity is None else np.ascontiguousarray(entity, np.uint32)
    st = np.zeros(len(seeds), _lib.DELIVERY_STATS_DTYPE)
    order = np.zeros((len(seeds), E), np.uint32)
    rel = np.zeros((len(seeds), E), np.int64)
    for i, s in enumerate(seeds):
        b = s.encode()
        sb = np.frombuffer(b, np.uint8) if b else np.zeros(1, np.uint8)
        _lib.check(L.nmz_replayable_delivery_host(_lib.ptr(sb), len(b), _lib.ptr(ho), _lib.ptr(hb), E, m,
                                                  _lib.ptr(arr), _lib.ptr(sy), _lib.ptr(en), _lib.ptr(st[i:i + 1]),
                                                  _lib.ptr(order[i]), _lib.ptr(rel[i])))
    return st, order, rel


def same(got, exp):
    return np.asarray(got).tobytes() == np.asarray(exp).astype(np.asarray(got).dtype).tobytes() and \
        len(got) == len(exp)


def case_inputs(E, m, n_entities=0, none_every=0, rng_seed=0):
    """Hints, arrivals, symbols and entities of a random trace whose arrivals collide and interleave under m:
    arrivals are drawn from a range of about E * m / 4 (so neighbours overtake each other), in units that repeat
    (so releases tie when m is small), and never exceed 2^50."""
    rng = np.random.default_rng(rng_seed * 7919 + E * 31 + (m % 1000003))
    hints = [f"e{i}:{int(rng.integers(0, 1 << 30)):x}" for i in range(E)]
    span = int(min(2**50, max(8, (E * max(m, 1)) // 4)))
    arrival = rng.integers(0, span + 1, E, dtype=np.int64)
    arrival[::3] = arrival[::3] // 4 * 4  # repeated values among small spans
    if E > 2:
        arrival[2] = arrival[0]           # an equal-arrival pair
        arrival[E - 1] = span             # the largest value
    sym = rng.integers(0, 2**64, E, dtype=np.uint64)
    entity = None
    if n_entities:
        entity = rng.integers(0, n_entities, E).astype(np.uint32)
        if none_every:
            entity[none_every - 1::none_every] = NONE
    return hints, arrival, sym, entity
