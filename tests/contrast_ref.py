"""Numpy restatement of the order contrast ("Order contrast") and the generator of the test
storages. It shares nothing with the library: per run a boolean `p[:, None] < p[None, :]` masked by presence,
summed per label; the ranking is one lexsort on (index, -F, -score)."""
import functools

import numpy as np

NONE = 0xFFFFFFFF
INT64_MIN = -(1 << 63)

ORDER_PAIR_DTYPE = np.dtype([("before", "<u4"), ("after", "<u4"), ("score", "<i8"), ("n_fail_with", "<u4"),
                             ("n_pass_with", "<u4"), ("n_fail_against", "<u4"), ("n_pass_against", "<u4")])


def gen(E, R, seed):
    """pos[R][E] uint32, failed[R] uint8: each run a random order at positions permutation(E) * 3 + 1 (not dense),
    every (run, event) absent with probability 0.15 except events 7 % E and 3 % E, and a run fails iff it releases
    event 7 % E ahead of event 3 % E, flipped for 10 % of the runs; at least one run of each label."""
    rng = np.random.default_rng(seed)
    pos = np.stack([rng.permutation(E) for _ in range(R)]).astype(np.uint32) * 3 + 1
    absent = rng.random((R, E)) < 0.15
    absent[:, 7 % E] = False
    absent[:, 3 % E] = False
    pos[absent] = NONE
    noise = rng.random(R) < 0.10
    failed = ((pos[:, 7 % E] < pos[:, 3 % E]) ^ noise).astype(np.uint8)
    if not failed.any():
        failed[0] = 1
    if failed.all():
        failed[-1] = 0
    return pos, failed


@functools.lru_cache(maxsize=None)
def case(E, R):
    """gen(E, R, 1000 * E + R) with its counts, computed once and shared (read-only arrays)."""
    pos, failed = gen(E, R, 1000 * E + R)
    F, P = counts(pos, failed)
    for a in (pos, failed, F, P):
        a.setflags(write=False)
    return pos, failed, F, P


def counts(pos, failed):
    """F[b][a], P[b][a] (int32): failing / passing runs that hold both events and release b ahead of a."""
    pos = np.asarray(pos, np.uint32)
    R, E = pos.shape
    F = np.zeros((E, E), np.int32)
    P = np.zeros((E, E), np.int32)
    for r in range(R):
        p = pos[r]
        here = p != NONE
        lt = (p[:, None] < p[None, :]) & here[:, None] & here[None, :]
        if failed[r]:
            F += lt
        else:
            P += lt
    return F, P


def scores(F, P, failed):
    n_fail = int(np.count_nonzero(failed))
    n_pass = len(failed) - n_fail
    return F.astype(np.int64) * n_pass - P.astype(np.int64) * n_fail


def ranked(F, P, failed, k):
    """(pairs[k] as ORDER_PAIR_DTYPE with sentinels, n_positive): (score desc, F desc, b * E + a asc), score > 0."""
    E = F.shape[0]
    sc = scores(F, P, failed).reshape(-1)
    Ff = F.reshape(-1).astype(np.int64)
    idx = np.nonzero(sc > 0)[0]
    n_positive = len(idx)
    if n_positive > k:
        # nothing below the k-th best score can be listed: the sort then runs over the rest only
        kth = np.partition(sc[idx], n_positive - k)[n_positive - k]
        idx = idx[sc[idx] >= kth]
    order = idx[np.lexsort((idx, -Ff[idx], -sc[idx]))][:k]
    out = np.zeros(k, ORDER_PAIR_DTYPE)
    out["before"] = NONE
    out["after"] = NONE
    out["score"] = INT64_MIN
    n = len(order)
    b, a = order // E, order % E
    out["before"][:n] = b
    out["after"][:n] = a
    out["score"][:n] = sc[order]
    out["n_fail_with"][:n] = F[b, a]
    out["n_pass_with"][:n] = P[b, a]
    out["n_fail_against"][:n] = F[a, b]
    out["n_pass_against"][:n] = P[a, b]
    return out, n_positive


def one_pair(F, P, failed, b, a):
    """The record order_pair gives for (b, a)."""
    sc = scores(F, P, failed)
    return (b, a, int(sc[b, a]), int(F[b, a]), int(P[b, a]), int(F[a, b]), int(P[a, b]))
