"""Trace families for the move-profile tests (not a test module): the random family whose scripts hold moves in both
directions, repeated values and unequal DEL / INS counts (the rotations that partner the last slot of a full band
are in tests/golden/move_profile_kat.json). Pure Python lists of small ints; `encode` makes the u64 symbols the
library takes, `host_scripts` the scripts of nmz_ed_align_host that the expected profiles are computed over."""
import functools
import random

import numpy as np

GOLDEN = np.uint64(0x9E3779B97F4A7C15)
SEED = 2025
LENGTHS = (0, 1, 31, 64, 65, 130)


def encode(ids):
    """Dense symbol ids -> u64 event hashes (increasing ids do not give increasing hashes)."""
    return np.asarray(ids, np.int64).astype(np.uint64) * GOLDEN + np.uint64(5)


def encode_one(v):
    return int(encode([v])[0])


@functools.lru_cache(maxsize=None)
def family(w):
    """30 traces: per length the prefix of one base of 130 elements over 4 symbols; the prefix with 1, 3 and 6
    elements each popped and re-inserted up to w/2, w/4 and w/8 places away; the prefix with one element removed."""
    rng = random.Random(SEED)
    base = [rng.randrange(4) for _ in range(130)]
    out = []
    for L in LENGTHS:
        pre = base[:L]
        out.append(list(pre))
        for k, reach in ((1, w // 2), (3, w // 4), (6, w // 8)):
            t = list(pre)
            for _ in range(k):
                if len(t) < 2:
                    break
                i = rng.randrange(len(t))
                x = t.pop(i)
                t.insert(min(max(i + rng.randint(-max(reach, 1), max(reach, 1)), 0), len(t)), x)
            out.append(t)
        t = list(pre)
        if t:
            t.pop(rng.randrange(len(t)))
        out.append(t)
    return tuple(tuple(t) for t in out)


def ordered_pairs(n):
    return [(i, j) for i in range(n) for j in range(n) if i != j]


def host_scripts(trs, pairs, w):
    """EditScripts of nmz_ed_align_host over pairs of the u64 traces `trs`: all `w` slots, sentinels included."""
    import ctypes

    from namazu_amd import _lib, historystorage as hs
    dist = np.zeros(len(pairs), np.uint32)
    ops = np.zeros((len(pairs), w), _lib.EDIT_OP_DTYPE)
    memo = {}
    for p, (i, j) in enumerate(np.asarray(pairs).reshape(-1, 2).tolist()):
        if (i, j) not in memo:
            a, b = np.ascontiguousarray(trs[i], np.uint64), np.ascontiguousarray(trs[j], np.uint64)
            d, o = ctypes.c_uint32(), np.zeros(w, _lib.EDIT_OP_DTYPE)
            _lib.check(_lib.load().nmz_ed_align_host(_lib.ptr(a), len(a), _lib.ptr(b), len(b), w, ctypes.byref(d),
                                                     _lib.ptr(o) if w else None))
            memo[(i, j)] = (d.value, o)
        dist[p], ops[p] = memo[(i, j)]
    return hs.EditScripts(dist, ops, w)
