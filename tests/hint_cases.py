"""Replay hints as real traces carry them -- long, non-ASCII, at every byte alignment -- with a plain reference of
the replayable policy's delays (not a test module).

    delay(seed, hint) = FNV-1a 64 (seed || hint) % uint64(m)          (0 when m == 0)

The reference takes any string as a hint (signal/event.go:47-58: replay_hint is whatever the inspector set): 40- or
64-character digests, JSON fragments, UTF-8 text. reference_delays restates the definition in numpy uint64 arrays over
the seeds, one xor and one multiply per hint byte; reference_delays_py in Python integers. Neither uses the C oracle
or the library. Every hint family is built so that the property it is there for holds, and states the property in a
function of its own (tests/test_hint_bytes.py asserts them on the CPU). Everything is an integer: tests compare with
equality."""
import functools

import numpy as np

FNV_OFFSET = 0xCBF29CE484222325
FNV_PRIME = 0x100000001B3
MASK64 = 2**64 - 1
NONE = 0xFFFFFFFF
WT_BRUTE = 8  # csrc/replayable_wt_dev.h: classes of at most this many events take no wavelet-tree image
STATS_DTYPE = np.dtype([("sum_delay_ns", "<u8"), ("max_delay_ns", "<i8"), ("argmax_event", "<u4")])

# the moduli of the CPU parity test: small, the sweep's usual one, either side of 2^31 and 2^32, the largest int64,
# zero (every delay 0) and -1 (uint64(m) = 2^64 - 1)
M_ALL = (7, 10**8, 2**30 + 5, 2**31 + 3, 2**32 + 7, 2**63 - 1, 0, -1)


# ---------------------------------------------------------------- the reference
def _as_bytes(x):
    return x.encode() if isinstance(x, str) else bytes(x)


@functools.lru_cache(maxsize=32)
def _hashes(seeds, hints):
    """FNV-1a 64 of seed || hint for every pair: uint64[S, E], computed once per (seeds, hints) and read-only."""
    S, E = len(seeds), len(hints)
    prime = np.uint64(FNV_PRIME)
    h0 = np.full(S, FNV_OFFSET, np.uint64)
    lens = np.array([len(s) for s in seeds], np.int64)
    pad = np.zeros((S, int(lens.max()) if S else 0), np.uint64)
    for i, s in enumerate(seeds):
        pad[i, :len(s)] = np.frombuffer(s, np.uint8)
    out = np.zeros((S, E), np.uint64)
    with np.errstate(over="ignore"):
        for k in range(pad.shape[1]):
            h0 = np.where(k < lens, (h0 ^ pad[:, k]) * prime, h0)
        h = np.empty(S, np.uint64)
        for e, hint in enumerate(hints):
            np.copyto(h, h0)
            for b in hint:
                np.bitwise_xor(h, np.uint64(b), out=h)
                np.multiply(h, prime, out=h)
            out[:, e] = h
    out.setflags(write=False)
    return out


def reference_delays(seeds, hints, m):
    """int64[S, E]: FNV-1a 64 over seed || hint, then % uint64(m) (0 when m == 0), as the int64 the ABI returns.
    The result is read-only: tests share it."""
    h = _hashes(tuple(_as_bytes(s) for s in seeds), tuple(_as_bytes(x) for x in hints))
    mu = int(m) & MASK64
    out = (h % np.uint64(mu)).view(np.int64) if mu else np.zeros(h.shape, np.int64)
    out.setflags(write=False)
    return out


def reference_delays_py(seeds, hints, m):
    """reference_delays in Python integers, for spot checks."""
    mu = int(m) & MASK64
    out = np.zeros((len(seeds), len(hints)), np.int64)
    for i, s in enumerate(seeds):
        h0 = FNV_OFFSET
        for b in _as_bytes(s):
            h0 = ((h0 ^ b) * FNV_PRIME) & MASK64
        for e, x in enumerate(hints):
            h = h0
            for b in _as_bytes(x):
                h = ((h ^ b) * FNV_PRIME) & MASK64
            d = h % mu if mu else 0
            out[i, e] = d - 2**64 if d >= 2**63 else d
    return out


def reference_stats(delays):
    """sum_delay_ns (mod 2^64), max_delay_ns (as int64) and argmax_event (the first event index that attains the
    maximum) per seed, as the sweep's statistics define them."""
    d = np.asarray(delays, np.int64)
    st = np.zeros(d.shape[0], STATS_DTYPE)
    if d.shape[1] == 0:
        st["max_delay_ns"] = -2**63
        st["argmax_event"] = NONE
        return st
    with np.errstate(over="ignore"):
        st["sum_delay_ns"] = d.view(np.uint64).sum(axis=1, dtype=np.uint64)
    st["max_delay_ns"] = d.max(axis=1)
    st["argmax_event"] = d.argmax(axis=1)  # the first maximum
    return st


def hint_offsets(hints):
    """[E + 1] byte offsets of the hints in their CSR (the values of the hint_off the library receives)."""
    off = np.zeros(len(hints) + 1, np.int64)
    np.cumsum([len(h) for h in hints], out=off[1:])
    return off


def first_difference(got, exp, hints):
    """Where two delay matrices first differ, for a failure message: seed, event, the hint's length and the
    alignment of its first byte (hint_off[e] & 3)."""
    got, exp = np.asarray(got), np.asarray(exp)
    if got.shape != exp.shape:
        return f"shapes differ: {got.shape} != {exp.shape}"
    bad = np.argwhere(got != exp)
    if not len(bad):
        return "equal"
    s, e = (int(x) for x in bad[0])
    off = hint_offsets(hints)
    return (f"{len(bad)} delays differ, first at seed {s} event {e}: got {int(got[s, e])}, expected {int(exp[s, e])}; "
            f"hint length {len(hints[e])}, hint_off[e] & 3 = {int(off[e]) & 3}")


def stats_difference(got, exp, hints):
    """Where the sweep's statistics first differ from the expected records, for a failure message: the seed, the
    records, and the length and alignment of the hints of the two argmax events."""
    off = hint_offsets(hints)
    for s in range(min(len(got), len(exp))):
        if got[s] != exp[s]:
            def ev(e):
                e = int(e)
                return f"event {e} (hint length {len(hints[e])}, hint_off[e] & 3 = {int(off[e]) & 3})" \
                    if e < len(hints) else f"event {e}"
            return (f"stats differ first at seed {s}: got {got[s]}, expected {exp[s]}; argmax got "
                    f"{ev(got[s]['argmax_event'])}, expected {ev(exp[s]['argmax_event'])}")
    return "equal" if len(got) == len(exp) else f"lengths differ: {len(got)} != {len(exp)}"


# ---------------------------------------------------------------- seeds
@functools.lru_cache(maxsize=None)
def _seeds():
    rng = np.random.default_rng(0x5EED)
    out = [str(i).encode() for i in range(256)] + [b"", b"foobar", b"\xff" * 7, b"\x00"]
    while len(out) < 300:
        out.append(rng.integers(0, 256, int(rng.integers(0, 25)), dtype=np.uint8).tobytes())
    return tuple(out)


def seeds():
    """300 seeds as bytes: decimal 0..255, the empty seed (the reference's default), "foobar", 7 x 0xff, one NUL,
    and random bytes of length 0..24."""
    return list(_seeds())


# the online-decision tests' six seeds of seeds(): decimal, the empty seed, foobar, 0xff bytes, NUL, random bytes
DECIDE_SEEDS = (7, 256, 257, 258, 259, 299)


# ---------------------------------------------------------------- joints
JOINT_LENGTHS = (0, 1, 2, 3, 4, 5, 12, 13, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65, 100, 255, 256, 257, 1000)
JOINT_SMALL = (7, 20, 70)  # classes of 5: at or below WT_BRUTE
JOINT_PER_LENGTH, JOINT_PER_SMALL = 12, 5


def _special_hints(rng, length, n):
    """n hints of one length: all 0x00, all 0x80, all 0xff, two that differ only in their last byte, the rest
    uniform over 0..255."""
    if length == 0:
        return [b""] * n
    out = [bytes([0x00]) * length, bytes([0x80]) * length, bytes([0xff]) * length]
    a = rng.integers(0, 256, length, dtype=np.uint8)
    b = a.copy()
    b[-1] ^= 0x81  # the top and the bottom bit of the last byte
    out += [a.tobytes(), b.tobytes()]
    while len(out) < n:
        out.append(rng.integers(0, 256, length, dtype=np.uint8).tobytes())
    return out[:n]


@functools.lru_cache(maxsize=None)
def _joints():
    rng = np.random.default_rng(0x101)
    main = []
    for ln in JOINT_LENGTHS:
        main += _special_hints(rng, ln, JOINT_PER_LENGTH)
    for ln in JOINT_SMALL:
        main += _special_hints(rng, ln, JOINT_PER_SMALL)
    main = [main[i] for i in rng.permutation(len(main))]
    # spacers of 1..3 bytes steer the alignments: the i-th hint of a length of JOINT_LENGTHS (in event order) starts
    # at alignment i mod 4 for its first eight, so every alignment occurs twice at least in the class
    seen = {ln: 0 for ln in JOINT_LENGTHS}
    out, cur = [], 0
    for h in main:
        if len(h) in seen:
            i = seen[len(h)]
            seen[len(h)] += 1
            if i < 8:
                gap = (i - cur) & 3
                if gap:
                    out.append(rng.integers(0, 256, gap, dtype=np.uint8).tobytes())
                    cur += gap
        out.append(h)
        cur += len(h)
    # the trace ends in a spacer, at a total of 1 (mod 4): the last dword of the hint bytes is a partial one
    for gap in ((1, 3) if (1 - cur) & 3 == 0 else ((1 - cur) & 3,)):
        out.append(rng.integers(0, 256, gap, dtype=np.uint8).tobytes())
        cur += gap
    return tuple(out)


def joints():
    """The fused reader's lengths at every start alignment: 12 hints of every length of JOINT_LENGTHS (classes above
    WT_BRUTE) and 5 of every length of JOINT_SMALL, in a shuffled order, with spacer hints of 1..3 bytes between them
    so that every class of 12 holds each start alignment twice; bytes uniform over 0..255, per length one hint all
    0x00, one all 0x80, one all 0xff and two that differ in their last byte only. The total is 1 (mod 4)."""
    return list(_joints())


def joints_tail(r):
    """joints() with its last hint (a spacer) lengthened so that the total byte count is r (mod 4)."""
    out = list(_joints())
    extra = (r - 1) & 3
    out[-1] = out[-1] + bytes([0xA5, 0x00, 0xFE][:extra])
    return out


def check_joints(hints, r=1):
    """The properties joints() / joints_tail(r) are there for; returns the number of 16-byte rounds the fused reader
    runs on the longest class above WT_BRUTE."""
    off = hint_offsets(hints)
    assert int(off[-1]) % 4 == r, f"total bytes {int(off[-1])} is not {r} (mod 4)"
    assert len(hints[-1]) > 0, "the last hint is empty: the last word clamp would not see the partial dword"
    lens = np.array([len(h) for h in hints])
    # straight from the data: the longest hint length that more than WT_BRUTE events share, in rounds of 16 bytes
    rounds = (max(ln for ln, n in class_sizes(hints).items() if n > WT_BRUTE) + 15) // 16
    for ln in JOINT_LENGTHS:
        ev = np.nonzero(lens == ln)[0]
        assert len(ev) >= JOINT_PER_LENGTH > WT_BRUTE, f"length {ln}: {len(ev)} hints"
        al = np.bincount(off[ev] & 3, minlength=4)
        assert (al >= 2).all(), f"length {ln}: start alignments {al.tolist()}"
        if ln:
            have = {bytes(hints[e]) for e in ev}
            for v in (0x00, 0x80, 0xff):
                assert bytes([v]) * ln in have, f"length {ln}: no hint of all {v:#04x}"
            assert any(a[:-1] == b[:-1] and a[-1] != b[-1] for a in have for b in have), \
                f"length {ln}: no two hints that differ in the last byte only"
    for ln in JOINT_SMALL:
        assert 0 < int((lens == ln).sum()) <= WT_BRUTE, f"length {ln}: not a class at or below WT_BRUTE"
    body = np.frombuffer(b"".join(hints), np.uint8)
    assert len(np.unique(body)) == 256, "some byte value never occurs"
    return rounds


# ---------------------------------------------------------------- one long hint
@functools.lru_cache(maxsize=None)
def _one_long(E, extra):
    rng = np.random.default_rng(E * 16 + extra)
    out = [rng.integers(0, 256, int(rng.integers(3, 31)), dtype=np.uint8).tobytes() for _ in range(E - 1)]
    out.insert(E // 2, rng.integers(0, 256, 4 * E + 4096 + extra, dtype=np.uint8).tobytes())
    return tuple(out)


def one_long(E, extra):
    """E - 1 hints of 3..30 bytes and, in the middle, one of 4 E + 4096 + extra bytes: with extra = 1 plan_create
    sorts the hints by a comparison sort, with extra = 0 by its counting sort with the largest position vector."""
    return list(_one_long(E, extra))


def takes_comparison_sort(hints):
    """plan_create's branch (csrc/replayable.hip): maxlen > 4 E + 4096."""
    return max(len(h) for h in hints) > 4 * len(hints) + 4096


# ---------------------------------------------------------------- class structure
@functools.lru_cache(maxsize=None)
def _many_classes():
    rng = np.random.default_rng(700)
    out = [rng.integers(0, 256, ln, dtype=np.uint8).tobytes() for ln in range(700)]
    return tuple(out[i] for i in rng.permutation(700))


def many_classes():
    """700 hints of lengths 0..699, one each, shuffled: 700 classes of 1."""
    return list(_many_classes())


@functools.lru_cache(maxsize=None)
def _mid_classes():
    rng = np.random.default_rng(90)
    out = [rng.integers(0, 256, ln, dtype=np.uint8).tobytes() for ln in range(10, 190, 2) for _ in range(9)]
    return tuple(out[i] for i in rng.permutation(len(out)))


def mid_classes():
    """90 lengths (every second from 10 to 188) with 9 hints each, shuffled: 90 classes just above WT_BRUTE."""
    return list(_mid_classes())


@functools.lru_cache(maxsize=None)
def _long_class():
    rng = np.random.default_rng(4097)
    return tuple(rng.integers(0, 256, 64, dtype=np.uint8).tobytes() for _ in range(4097))


def long_class():
    """4,097 hints of exactly 64 random bytes: one class, two wavelet-tree sub-segments, four full rounds."""
    return list(_long_class())


def class_sizes(hints):
    """{hint length: number of hints} -- the plan's length classes."""
    lens, counts = np.unique([len(h) for h in hints], return_counts=True)
    return dict(zip(lens.tolist(), counts.tolist()))


FAMILIES = {
    "joints": joints,
    "joints_tail2": lambda: joints_tail(2),
    "joints_tail3": lambda: joints_tail(3),
    "joints_tail0": lambda: joints_tail(0),
    "one_long_5_0": lambda: one_long(5, 0),
    "one_long_5_1": lambda: one_long(5, 1),
    "one_long_300_0": lambda: one_long(300, 0),
    "one_long_300_1": lambda: one_long(300, 1),
    "many_classes": many_classes,
    "mid_classes": mid_classes,
    "long_class": long_class,
}


def family_seeds(name):
    """The seeds a family is swept with: seeds(), or its first 64 for long_class (4,097 x 64 bytes per seed)."""
    return seeds()[:64] if name == "long_class" else seeds()


# ---------------------------------------------------------------- the sweeps that build their tables on the host
HOST_M = 10**8
HOST_SEED_LO, HOST_N_SEEDS = 990, 300  # decimal seeds 990 .. 1289: the range crosses 999 -> 1000


def host_sweep_seeds():
    return [str(HOST_SEED_LO + i) for i in range(HOST_N_SEEDS)]


def order_constraints(hints):
    """8 constraints over events of the 1,000-, 257-, 64-, 16- and 0-byte hints of joints(), margins 1 ns and 1 ms."""
    lens = np.array([len(h) for h in hints])
    ev = {ln: [int(e) for e in np.nonzero(lens == ln)[0][:2]] for ln in (1000, 257, 64, 16, 0)}
    a, b = 0, 1
    pairs = [(ev[1000][a], ev[257][a]), (ev[257][a], ev[64][a]), (ev[64][a], ev[16][a]), (ev[16][a], ev[0][a]),
             (ev[0][a], ev[1000][b]), (ev[1000][b], ev[64][b]), (ev[257][b], ev[16][b]), (ev[0][b], ev[1000][a])]
    return [(x, y, 1 if i % 2 == 0 else 10**6) for i, (x, y) in enumerate(pairs)]
