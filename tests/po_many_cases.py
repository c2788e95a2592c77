"""The PO family over hundreds of populated entities (not a test module).

68 traces of 650 .. 1,000 elements, each a random interleaving of the sequences of 200 entities, about 3 % of the
elements on NMZ_NONE. Under the map "g1024" (n_entities = 1,024) the populated ids are the joints of the kernels'
layouts -- k_po_knn's chunks of 64, k_po_gather's four entities per thread and 64 threads per wave, the profile's fold
by 32 -- and random others; "dense" replaces every id by its rank and takes n_entities = 203, which is no multiple of 4
or 64. Every id of 41 .. 71 and of 701 .. 731 is populated, so the pairs 40 / 72 and 700 / 732 are 32 ranks apart and
share a lenfold word under both maps.

The variants (PO-unequal to the base only where stated):
  base, plain{i}   31 interleavings of the same per-entity sequences: PO distance 0.
  chunk{c}_{t}     t in {1, 5, 9, 33} random SUB / INS / DEL edits inside the entities with id // 64 == c in {0, 1, 7, 15}.
  spread{t}        one substitution in each of t in {8, 9, 16, 32, 33, 64, 65} entities spread evenly over the populated
                   ids, the last of them 1023: exactly t from the base, the last edit in the last chunk.
  foldbase         the base with entity 40 at 40 elements and entity 72 empty;
  fold{x}          foldbase with entity 40 at its first 40 - x elements and entity 72 at the first x of one fixed
                   sequence, x in {3, 5, 10, 17, 33, 38}: LB_len 0 and distance = length sum = 2 |x - y| between any two.
  sat{n1}_{n2}     the base with n1 copies of one symbol in entity 700 and n2 of another in 732: one gram bucket at 255,
                   256 .. 320 rows of one entity behind the 120 tiny ones below it. sat200_100 keeps both buckets
                   below 255: against sat300_0 LB_len is 0 and LB_gram 39 only because the other side stops at 255.

tests/test_po_many_host.py ties the host forms to the definition on this family, makes the distances, the lower bounds
and the length sums of every ordered pair from them and asserts that the family is not vacuous;
tests/test_po_many_gpu.py compares the kernels with those. `passing_chunk` says, by a plain Levenshtein per entity, in
which chunk of 64 entities a pair's running sum passes the band."""
import functools

import numpy as np

import ed_cases as EC
from namazu_amd import _lib

NONE = _lib.NMZ_NONE
JOINTS = (0, 31, 32, 63, 64, 65, 127, 128, 255, 256, 257, 511, 512, 767, 768, 1022, 1023)
N_POPULATED = 200
MAPS = {"g1024": 1024, "dense": 203}
N_PLAIN = 30
CHUNKS, CHUNK_EDITS = (0, 1, 7, 15), (1, 5, 9, 33)
SPREAD = (8, 9, 16, 32, 33, 64, 65)
FOLD, FOLD_A, FOLD_B, FOLD_LEN = (3, 5, 10, 17, 33, 38), 40, 72, 40
SAT, SAT_A, SAT_B = ((300, 0), (290, 0), (256, 44), (260, 40), (320, 0), (299, 1), (200, 100)), 700, 732
NONE_SHARE = 0.03
KINDS = ("base", "plain", "chunk", "spread", "foldbase", "fold", "sat")


def kind(name):
    return name.rstrip("0123456789_") if name != "foldbase" else name


@functools.lru_cache(maxsize=None)
def populated():
    """The 200 populated ids under "g1024", ascending."""
    rng = np.random.default_rng(2001)
    ids = set(JOINTS) | set(range(FOLD_A, FOLD_B + 1)) | set(range(SAT_A, SAT_B + 1))
    for c in CHUNKS:  # every edited chunk holds entities beside its joints
        free = [g for g in range(64 * c, 64 * c + 64) if g not in ids]
        ids |= set(rng.choice(free, size=6, replace=False).tolist())
    free = [g for g in range(1024) if g not in ids]
    ids |= set(rng.choice(free, size=N_POPULATED - len(ids), replace=False).tolist())
    out = tuple(sorted(int(g) for g in ids))
    assert len(out) == N_POPULATED and out.index(FOLD_B) - out.index(FOLD_A) == 32
    assert out.index(SAT_B) - out.index(SAT_A) == 32
    return out


def _sym(g, rng, n=1):
    """n dense symbols of entity g's private alphabet {4 g .. 4 g + 3}."""
    return [4 * g + int(x) for x in rng.integers(0, 4, size=n)]


def _edit(seqs, pool, n_edits, rng):
    """n_edits random SUB / INS / DEL inside the entities of `pool`; a SUB changes the symbol."""
    seqs = {g: list(s) for g, s in seqs.items()}
    for _ in range(n_edits):
        g = int(pool[int(rng.integers(0, len(pool)))])
        s, op = seqs[g], int(rng.integers(0, 3))
        if op == 0 and s:
            p = int(rng.integers(0, len(s)))
            s[p] = 4 * g + (s[p] - 4 * g + 1 + int(rng.integers(0, 3))) % 4
        elif op == 1 and s:
            del s[int(rng.integers(0, len(s)))]
        else:
            s.insert(int(rng.integers(0, len(s) + 1)), _sym(g, rng)[0])
    return seqs


def _interleave(seqs, rng):
    """One random interleaving of the entities' sequences with NONE_SHARE of NMZ_NONE elements: (symbols, ids)."""
    gs = [g for g in sorted(seqs) for _ in seqs[g]]
    n_none = int(round(len(gs) * NONE_SHARE / (1 - NONE_SHARE)))
    order = rng.permutation(np.array(gs + [NONE] * n_none, np.int64))
    at = dict.fromkeys(seqs, 0)
    sym = []
    for g in order.tolist():
        if g == NONE:
            sym.append(4096 + int(rng.integers(0, 4)))
        else:
            sym.append(seqs[g][at[g]])
            at[g] += 1
    return EC.encode(sym), order.astype(np.uint32)


@functools.lru_cache(maxsize=None)
def family():
    """(names, traces, entities under "g1024"), the per-entity sequences of every trace beside them."""
    rng = np.random.default_rng(2002)
    ids = populated()
    base = {g: _sym(g, rng, int(L)) for g, L in zip(ids, rng.choice(np.arange(1, 7), size=len(ids),
                                                                 p=(0.2, 0.2, 0.18, 0.16, 0.14, 0.12)))}
    rows = [("base", base)] + [("plain%d" % i, base) for i in range(N_PLAIN)]
    for c in CHUNKS:
        pool = [g for g in ids if g // 64 == c]
        rows += [("chunk%d_%d" % (c, t), _edit(base, pool, t, rng)) for t in CHUNK_EDITS]
    for t in SPREAD:
        seqs = {g: list(s) for g, s in base.items()}
        picks = sorted({ids[int(round(x))] for x in np.linspace(0, len(ids) - 1, t)})
        assert len(picks) == t and picks[-1] == 1023
        for g in picks:
            p = int(rng.integers(0, len(seqs[g])))
            seqs[g][p] = 4 * g + (seqs[g][p] - 4 * g + 1 + int(rng.integers(0, 3))) % 4
        rows.append(("spread%d" % t, seqs))
    fold = dict(base)
    fold[FOLD_A], fold[FOLD_B] = _sym(FOLD_A, rng, FOLD_LEN), []
    moved = _sym(FOLD_B, rng, FOLD_LEN)
    rows.append(("foldbase", fold))
    for x in FOLD:
        seqs = dict(fold)
        seqs[FOLD_A], seqs[FOLD_B] = fold[FOLD_A][:FOLD_LEN - x], moved[:x]
        rows.append(("fold%d" % x, seqs))
    for n1, n2 in SAT:
        seqs = dict(base)
        seqs[SAT_A], seqs[SAT_B] = [4 * SAT_A] * n1, [4 * SAT_B + 1] * n2
        rows.append(("sat%d_%d" % (n1, n2), seqs))
    names = tuple(n for n, _ in rows)
    made = [_interleave(s, rng) for _, s in rows]
    assert len(names) == len(set(names)) >= 65 and {kind(n) for n in names} == set(KINDS)
    assert all(650 <= len(t) <= 1000 for t, _ in made), sorted(len(t) for t, _ in made)
    return names, tuple(t for t, _ in made), tuple(e for _, e in made), tuple(s for _, s in rows)


@functools.lru_cache(maxsize=None)
def store(name):
    """(names, traces, entities, n_entities) under the map `name`."""
    names, trs, ents, _ = family()
    if name == "dense":
        ids = np.array(populated(), np.uint32)
        ents = tuple(np.where(e == NONE, NONE, np.searchsorted(ids, e)).astype(np.uint32) for e in ents)
    return names, trs, ents, MAPS[name]


def to_map(name, g):
    """The id under the map `name` of the "g1024" id g."""
    return populated().index(g) if name == "dense" else g


def index_of(trace_name):
    return family()[0].index(trace_name)


# 18 traces with every variant kind: the pairs of the script tests
SAMPLE = ("base", "plain0", "plain1", "chunk0_5", "chunk1_9", "chunk7_33", "chunk15_1", "chunk15_9", "spread8",
          "spread9", "spread33", "spread65", "foldbase", "fold5", "fold33", "sat300_0", "sat256_44", "sat260_40")
# six of them: 30 ordered pairs at band 1,024
SAMPLE_WIDEST = ("base", "chunk7_33", "spread65", "fold33", "sat300_0", "sat256_44")


def ordered_pairs(trace_names, with_self=True):
    idx = [index_of(n) for n in trace_names]
    return np.array([[i, j] for i in idx for j in idx if with_self or i != j], np.uint32)


# ---- the entities of a pair one by one, by the definition (lists and ints only) -----------------------------------------
@functools.lru_cache(maxsize=None)
def lev(a, b):
    """Levenshtein distance of two tuples by the two-row recurrence."""
    if a == b:
        return 0
    row = list(range(len(b) + 1))
    for i, x in enumerate(a, 1):
        new = [i]
        for j, y in enumerate(b, 1):
            new.append(min(row[j - 1] + (x != y), row[j] + 1, new[j - 1] + 1))
        row = new
    return row[-1]


def entity_distances(i, j):
    """[(g, Lev(i|g, j|g))] over the "g1024" ids ascending, entities that differ only."""
    si, sj = family()[3][i], family()[3][j]
    out = []
    for g in populated():
        if si[g] != sj[g]:
            out.append((g, lev(tuple(si[g]), tuple(sj[g]))))
    return out


def passing_chunk(name, i, j, w):
    """The chunk (id // 64 under the map `name`) in which the running sum of the entities' distances, ascending, first
    passes w; None when it never does."""
    total = 0
    for g, d in entity_distances(i, j):
        total += d
        if total > w:
            return to_map(name, g) // 64
    return None
