"""The probe traces of the signature tests and the crafted inputs of the class tests (not a test module).

Every probe is a deterministic function of (pattern, n, B): an entity pattern over the positions 0..n-1 under the
entity bound B, and n symbols drawn with a fixed seed from one pool of 64 uint64 values that holds 0 and 2^64 - 1
(a small pool: the same symbol meets many ranks, so a wrong rank changes the sum). The lengths sit around the
kernel's 64-lane steps and 256-element batches; the long ones pass rank 65,535, the end of the key table.
A call is the probes of one bound in a fixed shuffled order (the four waves of a workgroup hold different lengths,
empty traces included), trimmed so that N % 4 takes 1, 2 and 3 over the bounds (the wave tail t >= N)."""
import functools

import numpy as np

import sig_ref

NONE = sig_ref.NONE
M64 = sig_ref.M64
PATTERNS = ("one", "distinct64", "alt2", "blocks37", "returning", "none_mixed", "all_none", "top_id", "top_bit",
            "random")
SHORT = (0, 1, 63, 64, 65, 255, 256, 257, 511, 513, 1000)
LONG = (65535, 65536, 65537, 70000)
LONG_PATTERNS = ("one", "alt2")
BOUNDS = (1, 7, 64, 65, 1024, 1025, 4096, 4097, 16384)
# sig_launch's thresholds (csrc/unique.hip): LDS masks up to 1,024 entities, ballots with 4 waves per workgroup up to
# 4,096, ballots with 1 wave per workgroup up to 16,384
SIG_MASK_ENT, SIG_MAX_ENT_LDS, SIG_MAX_ENT = 1024, 4096, 16384


@functools.lru_cache(maxsize=None)
def pool():
    rng = np.random.default_rng(0x51C)
    p = rng.integers(0, 2**64, 64, dtype=np.uint64)
    p[5], p[41] = 0, M64
    return p


def _seed(*key):
    return [PATTERNS.index(k) if k in PATTERNS else int(k) for k in key]


def entities(pattern, n, B):
    """uint32 entity ids of the pattern over positions 0..n-1, every id < B or NMZ_NONE."""
    i = np.arange(n, dtype=np.int64)
    if pattern == "one":
        e = np.zeros(n, np.int64)
    elif pattern == "distinct64":
        e = i % min(64, B)
    elif pattern == "alt2":
        e = i % min(2, B)
    elif pattern == "blocks37":
        e = (i // 37) % min(5, B)
    elif pattern == "returning":
        e = i % min(7, B)
        e[::200] = min(3, B - 1)
    elif pattern == "none_mixed":
        e = (i * i) % min(11, B)
        e[i % 3 == 1] = NONE
    elif pattern == "all_none":
        e = np.full(n, NONE, np.int64)
    elif pattern == "top_id":
        e = np.where(i % 2 == 0, B - 1, 0)
    elif pattern == "top_bit":
        # two ids that differ in the top bit of B - 1 alone: the last of the ballots must separate them
        top = B - 1
        e = np.where(i % 2 == 0, top, top & ~(1 << max(top.bit_length() - 1, 0)))
    elif pattern == "random":
        e = np.random.default_rng(_seed(pattern, n, B)).integers(0, min(B, 300), n)
    else:
        raise ValueError(pattern)
    assert ((e < B) | (e == NONE)).all()
    return e.astype(np.uint32)


class Probe:
    """One trace: sym[n] uint64, ent[n] uint32 or None (exact mode)."""

    def __init__(self, name, sym, ent):
        self.name, self.sym, self.ent = name, sym, ent

    def __len__(self):
        return len(self.sym)

    def __repr__(self):
        return self.name


@functools.lru_cache(maxsize=None)
def probe(pattern, n, B):
    """The probe (pattern, n) under bound B. The long probes' ids do not depend on B (B >= 2 for alt2), so their
    symbols do not either: one restatement serves every call that holds them."""
    long = n in LONG
    sym = pool()[np.random.default_rng(_seed(pattern, n, 0 if long else B) + [1]).integers(0, 64, n)]
    return Probe(f"{pattern}[{n}]@{B}", sym, entities(pattern, n, B))


@functools.lru_cache(maxsize=None)
def exact_probe(n, k):
    sym = pool()[np.random.default_rng([n, k, 2]).integers(0, 64, n)]
    return Probe(f"exact{k}[{n}]", sym, None)


def _shuffled(probes, keep, drop):
    """A fixed shuffle; `drop` of the probes for which keep() is false leave, from the end of the order."""
    order = np.random.default_rng(len(probes)).permutation(len(probes))
    out = [probes[i] for i in order]
    for i in range(len(out) - 1, -1, -1):
        if drop and not keep(out[i]):
            del out[i]
            drop -= 1
    assert drop == 0
    return out


@functools.lru_cache(maxsize=None)
def po_call(B, long=True):
    """The probes of one nmz_trace_signatures call in PO mode under bound B (top_id holds id B - 1)."""
    ps = [probe(p, n, B) for p in PATTERNS for n in SHORT]
    if long:
        ps += [probe(p, n, min(B, 2)) for p in LONG_PATTERNS for n in LONG]
    want = 1 + BOUNDS.index(B) % 3 if B in BOUNDS else 1  # N % 4
    drop = (len(ps) - want) % 4
    # only `random` probes leave: every other pattern keeps all its lengths
    return tuple(_shuffled(ps, lambda p: not p.name.startswith("random"), drop))


@functools.lru_cache(maxsize=None)
def exact_call():
    ps = [exact_probe(n, k) for n in SHORT for k in range(3)] + [exact_probe(n, 0) for n in LONG]
    return tuple(_shuffled(ps, lambda p: True, 0))


def csr(probes, po=True):
    """(off[N + 1] uint64, sym[total] uint64, ent[total] uint32 or None) of a call."""
    off = np.zeros(len(probes) + 1, np.uint64)
    off[1:] = np.cumsum([len(p) for p in probes])
    total = int(off[-1])
    sym = np.concatenate([p.sym for p in probes] + [np.zeros(0, np.uint64)]) if total else np.zeros(1, np.uint64)
    ent = None
    if po:
        ent = np.concatenate([p.ent for p in probes] + [np.zeros(0, np.uint32)]) if total else np.zeros(1, np.uint32)
        ent = np.ascontiguousarray(ent, np.uint32)
    return off, np.ascontiguousarray(sym, np.uint64), ent


_ref = {}


def reference(p, bound=None):
    """sig_ref.signature of a probe, computed once per (probe, bound) and shared by the tests of a session."""
    key = (id(p), bound)
    if key not in _ref:
        _ref[key] = (p, sig_ref.signature(p.sym, p.ent, bound))  # holds p: its id stays taken
    return _ref[key][1]


def bound_of(probes):
    """The entity bound nmz_trace_signatures derives: the largest id + 1."""
    b = 0
    for p in probes:
        if p.ent is not None and len(p.ent) and (p.ent != NONE).any():
            b = max(b, int(p.ent[p.ent != NONE].max()) + 1)
    return b


def step_profile(p):
    """Per 64-element step of a PO probe: (taken lanes, distinct entities, lanes of the largest group)."""
    out = []
    for c in range(0, len(p), 64):
        e = p.ent[c:c + 64]
        e = e[e != NONE].tolist()
        cnt = {}
        for x in e:
            cnt[x] = cnt.get(x, 0) + 1
        out.append((len(e), len(cnt), max(cnt.values()) if cnt else 0))
    return out


# ---- short probes for the literal loops -------------------------------------------------------------------------

def short_probes(n=240):
    """Short traces whose symbol determines the entity, as an event's hash does (the symbol of letter x under
    entity e is one fixed random value): traces of 0-6 elements over 3 entities and 2 letters, every fourth element
    without an event, and for every third trace a re-interleaving or an element swap of an earlier one. Equal and
    unequal pairs both abound. Returns [(entity or None, symbol)] lists."""
    rng = np.random.default_rng(77)
    table = rng.integers(1, 2**64, (3, 2), dtype=np.uint64)
    free = rng.integers(1, 2**64, 2, dtype=np.uint64)  # symbols of actions without an event
    out = []
    for i in range(n):
        if out and i % 3 == 2:
            t = list(out[int(rng.integers(len(out)))])
            if len(t) > 1:
                if i % 2:
                    a, b = rng.integers(len(t), size=2)
                    t[a], t[b] = t[b], t[a]
                else:
                    t = [t[k] for k in rng.permutation(len(t))]
        else:
            t = []
            for _ in range(int(rng.integers(0, 7))):
                if rng.random() < 0.25:
                    t.append((None, int(free[rng.integers(2)])))
                else:
                    e, x = int(rng.integers(3)), int(rng.integers(2))
                    t.append((e, int(table[e, x])))
        out.append(t)
    return out


# ---- crafted inputs of the class tests --------------------------------------------------------------------------

CLASS_SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 5000)
_X = 0x6A09E667F3BCC908
GRID = (0, 1, 1 << 63, M64, M64 - 1, _X, _X ^ 1, _X ^ (1 << 63))  # pairs differing in bit 0 only, in bit 63 only
GAPS = (0, 7, 7, 1 << 40, sig_ref.INT64_MAX)


def class_sigs(family, N):
    """[(lo, hi)] * N of a family, Python integers."""
    rng = np.random.default_rng([CLASS_FAMILIES.index(family), N])
    if family == "equal":
        return [(_X, M64 - 2)] * N
    if family == "distinct":
        # distinct in lo alone for even i and in hi alone for odd i: either half alone merges half of them
        return [((i * 0x9E3779B97F4A7C15) & M64, 3) if i % 2 == 0 else (3, (i * 0xC2B2AE3D27D4EB4F) & M64)
                for i in range(N)]
    if family == "grid":
        lo, hi = rng.integers(0, 8, N), rng.integers(0, 8, N)
        return [(GRID[a], GRID[b]) for a, b in zip(lo.tolist(), hi.tolist())]
    if family == "single_bit":
        assert N == 258
        vals = [0] + [1 << b for b in range(128)]
        both = [vals[i] for i in rng.permutation(np.repeat(np.arange(129), 2)).tolist()]
        return [(v & M64, v >> 64) for v in both]
    raise ValueError(family)


CLASS_FAMILIES = ("equal", "distinct", "grid", "single_bit")
CLASS_CASES = [(f, N) for f in CLASS_FAMILIES[:3] for N in CLASS_SIZES] + [("single_bit", 258)]


def class_gaps(family, N):
    rng = np.random.default_rng([CLASS_FAMILIES.index(family), N, 9])
    return [GAPS[k] for k in rng.integers(0, len(GAPS), N).tolist()]


def pair_agreement(sigs):
    """Unordered pairs that agree in hi only, in lo only, in both."""
    def pairs(keys):
        cnt = {}
        for k in keys:
            cnt[k] = cnt.get(k, 0) + 1
        return sum(c * (c - 1) // 2 for c in cnt.values())
    both = pairs(sigs)
    return pairs(hi for _, hi in sigs) - both, pairs(lo for lo, _ in sigs) - both, both
