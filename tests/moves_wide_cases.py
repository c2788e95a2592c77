"""Cases for the wide move-profile tests (not a test module): the constructed rows whose profile has a closed form
at any k, the moved-block family whose scripts run to 543 ops, and `host_scripts_wide`, the scripts of
nmz_ed_align_wide_host that the expected profiles are computed over. Pure Python lists of small ints; moves_cases'
`encode` makes the u64 symbols the library takes."""
import functools
import random

import numpy as np

import moves_cases as MC

X, Y = 1, 2
SUB, DEL, INS = 0, 1, 2
ZERO = dict.fromkeys(("later", "earlier", "dropped", "extra", "sub_from", "sub_to", "n_pairs", "reserved",
                      "span_later", "span_earlier"), 0)


def B(n):
    return list(range(10, 10 + n))


def constructed(k, j=3):
    """The rows of the table in DESIGN.md section 2, "Move profiles / Wider bands", at size k: dicts of name, a, b,
    band, dist, kinds (the script's op kinds, None beyond the band), partner (slot or None per op) and counts
    {symbol id: the nonzero counters}. Every script names X (and Y) in one pair: n_pairs = 1."""
    h = k // 2
    rows = [
        dict(name="rot", a=[X] * k + B(3 * k), b=B(3 * k) + [X] * k, band=2 * k, dist=2 * k,
             kinds=[DEL] * k + [INS] * k, partner=[s + k for s in range(k)] + list(range(k)),
             counts={X: dict(later=k, span_later=3 * k * k + k * (k - 1) // 2, n_pairs=1)}),
        dict(name="rot-rev", a=B(3 * k) + [X] * k, b=[X] * k + B(3 * k), band=2 * k, dist=2 * k,
             kinds=[INS] * k + [DEL] * k, partner=[s + k for s in range(k)] + list(range(k)),
             counts={X: dict(earlier=k, span_earlier=4 * k * k - k * (k - 1) // 2, n_pairs=1)}),
        dict(name="uneq", a=[X] * (k + j) + B(3 * k), b=B(3 * k) + [X] * (k - j), band=2 * k, dist=2 * k,
             kinds=[DEL] * (k + j) + [INS] * (k - j),
             partner=[s + k + j for s in range(k - j)] + [None] * (2 * j) + list(range(k - j)),
             counts={X: dict(later=k - j, dropped=2 * j, n_pairs=1,
                             span_later=3 * k * (k - j) + (k - j) * (k - j - 1) // 2)}),
        dict(name="xy", a=[X] * h + [Y] * (k - h) + B(3 * k), b=B(3 * k) + [Y] * (k - h) + [X] * h, band=2 * k,
             dist=2 * k, kinds=[DEL] * k + [INS] * k,
             partner=[2 * k - h + s for s in range(h)] + [k + s for s in range(k - h)]
             + [h + s for s in range(k - h)] + list(range(h)),
             counts={X: dict(later=h, n_pairs=1, span_later=sum(4 * k - h + s for s in range(h))),
                     Y: dict(later=k - h, n_pairs=1, span_later=sum(3 * k + s for s in range(k - h)))}),
        dict(name="rot-beyond", a=[X] * k + B(3 * k), b=B(3 * k) + [X] * k, band=2 * k - 1, dist=2 * k, kinds=None,
             partner=None, counts={}),
    ]
    for r in rows:
        r["counts"] = {v: dict(ZERO, **c) for v, c in r["counts"].items()}
        scripts = 0 if r["kinds"] is None else 1
        r["info"] = dict(n_scripts=scripts, n_beyond=1 - scripts, n_ops=r["dist"] * scripts, n_unknown=0)
    return rows


@functools.lru_cache(maxsize=None)
def family():
    """The moved-block family: 14 traces over 40 symbols. A base of 620 elements, its prefix of 560, and per block
    size k in (40, 150, 300, 480) the base with a block of k elements delivered later, one delivered earlier, and the
    first with 7 more elements dropped. Distances up to 543; one value moves up to 13 times in a script."""
    rng = random.Random(2026)
    base = [rng.randrange(40) for _ in range(620)]
    out = [list(base), base[:560]]
    for k in (40, 150, 300, 480):
        t = list(base); blk = t[20:20 + k]; del t[20:20 + k]; t[120:120] = blk          # noqa: E702 delivered later
        u = list(base); blk = u[600 - k:600]; del u[600 - k:600]; u[15:15] = blk        # noqa: E702 delivered earlier
        v = list(t)
        for _ in range(7):
            v.pop(rng.randrange(len(v)))
        out += [t, u, v]
    return tuple(tuple(t) for t in out)


_memo = {}


def wide_slots(a, b, w):
    """(dist, ops[w]) of nmz_ed_align_wide_host for one pair of u64 traces, kept per (traces, band)."""
    import ctypes

    from namazu_amd import _lib
    a, b = np.ascontiguousarray(a, np.uint64), np.ascontiguousarray(b, np.uint64)
    key = (a.tobytes(), b.tobytes(), w)
    if key not in _memo:
        d, o = ctypes.c_uint32(), np.zeros(w, _lib.EDIT_OP_DTYPE)
        _lib.check(_lib.load().nmz_ed_align_wide_host(_lib.ptr(a), len(a), _lib.ptr(b), len(b), w, ctypes.byref(d),
                                                      _lib.ptr(o) if w else None))
        _memo[key] = (d.value, o)
    return _memo[key]


def host_scripts_wide(trs, pairs, w):
    """MC.host_scripts through nmz_ed_align_wide_host: EditScripts over pairs of the u64 traces `trs`, all `w` slots,
    sentinels included; one alignment per distinct pair."""
    from namazu_amd import _lib, historystorage as hs
    pairs = np.asarray(pairs).reshape(-1, 2).tolist()
    dist = np.zeros(len(pairs), np.uint32)
    ops = np.zeros((len(pairs), w), _lib.EDIT_OP_DTYPE)
    for p, (i, j) in enumerate(pairs):
        dist[p], ops[p] = wide_slots(trs[i], trs[j], w)
    return hs.EditScripts(dist, ops, w)


@functools.lru_cache(maxsize=None)
def family_encoded():
    return tuple(MC.encode(t) for t in family())
