"""Reference for the ProcSetEvent decisions (helper, not a test file): a plain-Python restatement of the three
sub-policy loops (mild.go:44-57, extreme.go:44-63, dirichlet.go:58-82) and of the delay draw that precedes them
(util/queue/impl.go:110-128), over the oracle's Go generator. One decision is
O.GoRand(O.random_event_seed(seed, evhash)) drawing the delay, then the sub-policy's draws; nothing here calls the
library under test."""
import ctypes

import numpy as np

from oracle import oracle as O

MILD, EXTREME, DIRICHLET = 0, 1, 2
NORMAL, RR, BATCH, DEADLINE, RESET_ON_FORK = 0, 2, 3, 6, 1
NONE = 0xFFFFFFFF
M64 = (1 << 64) - 1

ATTR_DTYPE = np.dtype([("policy", "<u4"), ("nice", "<i4"), ("priority", "<u4"), ("flags", "<u4")])
STATS_DTYPE = np.dtype([("sum_delay_ns", "<u8"), ("score_sum", "<i8"), ("target_score", "<i8"),
                        ("n_special", "<u4"), ("flags", "<u4")])
TOPK_DTYPE = np.dtype([("seed", "<u8"), ("target_score", "<i8")])


class _GoRand(O.GoRand):
    """O.GoRand with the C functions and the state's reference looked up once per decision, not once per draw
    (a sweep's reference makes millions of draws)."""

    def __init__(self, seed):
        super().__init__(seed)
        L, ref = O.lib(), ctypes.byref(self._r)
        i31, i63, i = L.nmzo_go_int31n, L.nmzo_go_int63n, L.nmzo_go_intn
        self.int31n = lambda n: i31(ref, n)
        self.int63n = lambda n: i63(ref, n)
        self.intn = lambda n: i(ref, n)


class Params:
    """policy, PPPMild.UseBatch, PPPExtreme.Prioritized, int(PPPDirichlet.ResetProbability * 1000.0)"""

    def __init__(self, policy, use_batch=True, prioritized=3, reset_probability=0.1):
        self.policy = policy
        self.use_batch = bool(use_batch)
        self.prioritized = int(prioritized)
        self.reset_threshold = int(reset_probability * 1000.0)


def decide(seed, evhash, prioritized_entity, n_procs, rp, pp):
    """-> (delay, attrs[n_procs] as (policy, nice, priority, flags), scores[n_procs], n_special, outputs consumed).
    rp: O.random_params(...)."""
    r = _GoRand(O.random_event_seed(seed & M64, evhash))
    c = 1 if prioritized_entity else 0
    mn, mx = rp.min_ns[c], rp.max_ns[c]
    delay = mn if mn == mx else r.int63n(mx - mn) + mn
    attrs, scores, special = [], [], 0
    if pp.policy == MILD:
        for _ in range(n_procs):
            nice = -20 + r.int31n(40)
            attrs.append((BATCH if pp.use_batch else NORMAL, nice, 0, 0))
            scores.append(-nice)
            special += nice < 0
    elif pp.policy == EXTREME:
        prios = set()
        for _ in range(pp.prioritized):
            assert n_procs > 0, "Int31n(0) panics"
            prios.add(r.int31n(n_procs))
        for i in range(n_procs):
            if i in prios:
                pr = r.int31n(10)
                attrs.append((RR, 0, pr, 0))
                scores.append(1 + pr)
                special += 1
            else:
                attrs.append((BATCH, 0, 0, 0))
                scores.append(0)
    else:
        assert n_procs > 0, "has no process"
        for _ in range(n_procs):
            reset = r.intn(999) < pp.reset_threshold
            attrs.append((NORMAL, 0, 0, 0) if reset else (DEADLINE, 0, 0, RESET_ON_FORK))
            scores.append(int(reset))
            special += reset
    return delay, attrs, scores, special, r.n_out


def draws(n_procs, rp, pp, prioritized_entity, attrs):
    """Draws a decision makes when none is rejected (its outputs consumed are this, plus one per re-draw)."""
    c = 1 if prioritized_entity else 0
    d = 0 if rp.min_ns[c] == rp.max_ns[c] else 1
    if pp.policy == EXTREME:
        return d + max(pp.prioritized, 0) + sum(1 for a in attrs if a[0] == RR)
    return d + n_procs


def decide_events(seed, evhash, evclass, n_procs, rp, pp):
    """One seed over a list of events -> (delays int64[E], attrs ATTR_DTYPE[sum n_procs])."""
    delays, rows = [], []
    for h, c, n in zip(evhash, evclass, n_procs):
        d, a, _, _, _ = decide(seed, int(h), int(c) & 1, int(n), rp, pp)
        delays.append(d)
        rows.extend(a)
    return np.array(delays, np.int64), np.array(rows, ATTR_DTYPE) if rows else np.zeros(0, ATTR_DTYPE)


def sweep(seed0, n_seeds, evhash, evclass, n_procs, target_slot, rp, pp, n_dump=0, hits=None):
    """-> (stats STATS_DTYPE[n_seeds], delays int64[n_dump, E], attrs ATTR_DTYPE[n_dump, sum n_procs],
    outputs consumed [n_seeds, E]). hits, if given, is an int64[n_seeds, E] that receives the score of every event's
    target slot (0 without a target)."""
    E = len(evhash)
    total = int(sum(int(n) for n in n_procs))
    stats = np.zeros(n_seeds, STATS_DTYPE)
    delays = np.zeros((n_dump, E), np.int64)
    attrs = np.zeros((n_dump, total), ATTR_DTYPE)
    outs = np.zeros((n_seeds, E), np.int64)
    for i in range(n_seeds):
        seed = (seed0 + i) & M64
        sd = ss = ts = sp = 0
        off = 0
        for e in range(E):
            n = int(n_procs[e])
            d, a, sc, special, n_out = decide(seed, int(evhash[e]), int(evclass[e]) & 1, n, rp, pp)
            sd += d
            ss += sum(sc)
            sp += special
            t = NONE if target_slot is None else int(target_slot[e])
            if t != NONE:
                ts += sc[t]
                if hits is not None:
                    hits[i, e] = sc[t]
            outs[i, e] = n_out
            if i < n_dump:
                delays[i, e] = d
                if n:
                    attrs[i, off:off + n] = np.array(a, ATTR_DTYPE)
            off += n
        stats[i] = (sd & M64, ss, ts, sp, 0)
    return stats, delays, attrs, outs


def topk(stats, seed0, k, descending):
    """k best seeds by target_score (descending or ascending), then seed value ascending; padding
    {2^64 - 1, -2^63}."""
    seeds = [(seed0 + i) & M64 for i in range(len(stats))]
    ts = stats["target_score"].tolist()
    order = sorted(range(len(stats)), key=lambda i: (-ts[i] if descending else ts[i], seeds[i]))[:k]
    out = np.zeros(k, TOPK_DTYPE)
    out["seed"] = M64
    out["target_score"] = -(1 << 63)
    for j, i in enumerate(order):
        out[j] = (seeds[i], ts[i])
    return out
