"""Restatement of the order sweep's definition for the tests (not a test module).

Delays come from the C oracle (oracle.replayable_sweep with every seed dumped, or oracle.replayable_interval); the
definition of include/nmz_gpu.h is then applied in numpy:

    release[s][e] = arrival_ns[e] + delay[s][e]
    slack[s][c]   = release[s][after_c] - release[s][before_c] - margin_c        satisfied iff slack >= 0

and seeds are ranked by (n_satisfied desc, min_slack desc, seed asc). Everything is integer: tests compare with
equality."""
import functools

import numpy as np

from oracle import oracle as O

MS = 1_000_000
STATS_DTYPE = np.dtype([("sat_mask", "<u8"), ("min_slack_ns", "<i8"), ("n_satisfied", "<u4"),
                        ("argmin_constraint", "<u4")])
TOPK_DTYPE = O.TOPK_DTYPE
SENTINEL = (2**64 - 1, -(2**63), 0, 0xFFFFFFFF)

# fixture F of tests/golden/order_sweep_kat.json
F_HINTS = tuple(f"hint-entity-{i % 4}-{i}" for i in range(16))
F_ARRIVAL = tuple(i * 5 * MS for i in range(16))
# the fixture lists pairs (x, y, margin) of an earlier and a later arrival in which y has to overtake x: as
# (before, after, margin_ns) constraints that is before = y, after = x
F_PAIRS = ((0, 5, MS), (2, 9, MS), (3, 4, 1), (7, 12, 10 * MS), (1, 14, 1))
F_CONS = tuple((y, x, mg) for x, y, mg in F_PAIRS)
# the issue's moduli: 0, 1, a power of two, < 2^31, >= 2^32, the largest; 3e9 adds 2^31 <= m < 2^32
M_CASES = (0, 1, 2**20, 10**8, 9 * 10**9, 2**61, 3 * 10**9)


SEEDS = ["", "foobar"] + [str(i) for i in range(62)]  # the empty seed is the reference's default


def wide_constraints():
    """17 events and 64 constraints; the last is an equal-hint pair with room, so bit 63 of the mask is set for
    every seed. Returns (hints, arrival, constraints)."""
    rng = np.random.default_rng(64)
    cons = []
    while len(cons) < 63:
        b, a = (int(x) for x in rng.integers(0, 16, 2))
        if b != a:
            cons.append((b, a, int(rng.integers(1, 20 * MS))))
    hints = list(F_HINTS) + [F_HINTS[3]]
    arrival = list(F_ARRIVAL) + [F_ARRIVAL[3] + MS]
    return hints, arrival, cons + [(3, 16, 1)]


def decimal_seeds(lo, n):
    """The seed strings "lo" .. "lo + n - 1", wrapping past 2^64, and their integer values."""
    vals = [(lo + i) % 2**64 for i in range(n)]
    return [str(v) for v in vals], np.array(vals, np.uint64)


def delays(seeds, hints, m):
    """delay[s][e] for every seed and hint, from the C oracle's sweep dump."""
    so, sb = O.to_csr(list(seeds))
    ho, hb = O.to_csr(list(hints))
    if not len(seeds):
        return np.zeros((0, len(hints)), np.int64)
    return O.replayable_sweep(so, sb, ho, hb, m, n_dump=len(seeds))[1]


def slacks(dl, arrival, cons):
    rel = np.asarray(arrival, np.int64)[None, :] + dl
    c = np.asarray(cons, np.int64).reshape(-1, 3)
    return rel[:, c[:, 1]] - rel[:, c[:, 0]] - c[None, :, 2]


def stats_from_slack(sl):
    out = np.zeros(len(sl), STATS_DTYPE)
    sat = sl >= 0
    mask = np.zeros(len(sl), np.uint64)
    for c in range(sl.shape[1]):
        mask |= sat[:, c].astype(np.uint64) << np.uint64(c)
    out["sat_mask"] = mask
    out["n_satisfied"] = sat.sum(axis=1)
    if len(sl):
        out["min_slack_ns"] = sl.min(axis=1)
        out["argmin_constraint"] = sl.argmin(axis=1)  # the first minimum
    return out


def stats(seeds, hints, arrival, cons, m):
    return stats_from_slack(slacks(delays(seeds, hints, m), arrival, cons))


def topk(st, seed_values, k):
    """Best k by (n_satisfied desc, min_slack desc, seed value asc), sentinels past the seeds."""
    seed_values = np.asarray(seed_values, np.uint64)
    # |slack| < 2^63 by the limits, so the negations are exact
    order = np.lexsort((seed_values, -st["min_slack_ns"], -st["n_satisfied"].astype(np.int64)))[:k] \
        if len(st) else np.zeros(0, np.int64)
    out = np.zeros(k, TOPK_DTYPE)
    out[:] = SENTINEL
    out["seed"][:len(order)] = seed_values[order]
    out["sum_delay_ns"][:len(order)] = st["min_slack_ns"][order]
    out["n_fault"][:len(order)] = st["n_satisfied"][order]
    out["first_fault"][:len(order)] = st["argmin_constraint"][order]
    return out


@functools.lru_cache(maxsize=None)
def fixture_stats(m, lo=0, n=4096):
    """Fixture F over the decimal seeds lo .. lo + n - 1; computed once per (m, range) and shared, not modified."""
    st = stats(decimal_seeds(lo, n)[0], F_HINTS, F_ARRIVAL, F_CONS, m)
    st.setflags(write=False)
    return st


def host_order(seeds, hints, arrival, cons, m):
    """nmz_replayable_order_host for each seed string: (stats[len(seeds)], slack[len(seeds)][C])."""
    from namazu_amd import _lib
    from namazu_amd.explorepolicy import Replayable
    L = _lib.load()
    ho, hb = O.to_csr(list(hints))
    arr = np.ascontiguousarray(arrival, np.int64)
    cs = Replayable.order_constraints(cons)
    st = np.zeros(len(seeds), _lib.ORDER_STATS_DTYPE)
    sl = np.zeros((len(seeds), len(cs)), np.int64)
    for i, s in enumerate(seeds):
        sb = np.frombuffer(s.encode(), np.uint8) if s else np.zeros(1, np.uint8)
        _lib.check(L.nmz_replayable_order_host(_lib.ptr(sb), len(s.encode()), _lib.ptr(ho), _lib.ptr(hb), len(hints), m,
                                               _lib.ptr(arr), _lib.ptr(cs), len(cs), _lib.ptr(st[i:i + 1]),
                                               _lib.ptr(sl[i])))
    return st, sl


def same(got, exp):
    return np.array_equal(np.asarray(got).astype(exp.dtype), exp)
