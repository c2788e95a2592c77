"""CPU: the signature restatement (tests/sig_ref.py) and the probe set (tests/sig_cases.py) the GPU tests of
k_trace_sig and of the class builder rest on, checked without a device:

  * sig_ref against the numpy restatement of tests/delivery_ref.py (mix2 / fmix64) on the probe set;
  * sig_ref against the reference's literal loops (oracle.unique_curve_po / unique_curve_exact): signature equality
    <=> equality by the loops, pair by pair over short probes;
  * invariance under an injective relabelling of the entity ids; a trace with every element skipped has the empty
    trace's signature;
  * non-vacuity, computed from the probe set and the crafted class inputs alone;
  * nmz_trace_signatures / nmz_unique_traces refuse decreasing offsets before they look at the context."""
import numpy as np
import pytest

import delivery_ref as R
import sig_cases as C
import sig_ref
from namazu_amd import _lib
from oracle import oracle as O

U = np.uint64


def np_signature(sym, ent, bound=None):
    """The signature in numpy: ranks from a stable sort by entity, the sums through delivery_ref.mix2."""
    sym = np.asarray(sym, U)
    if ent is None:
        s, rank = sym, np.arange(len(sym), dtype=U)
    else:
        ent = np.asarray(ent, np.uint32)
        take = ent != C.NONE
        if bound is not None:
            take &= ent < bound
        s, e = sym[take], ent[take]
        o = np.argsort(e, kind="stable")
        es = e[o]
        rank = np.zeros(len(e), U)
        rank[o] = (np.arange(len(e)) - np.searchsorted(es, es, side="left")).astype(U)
    a, b = R.mix2(s, rank) if len(s) else (np.zeros(0, U), np.zeros(0, U))
    G = len(s)
    lo = a.sum(dtype=U, keepdims=True) + R.fmix64(U(G + 1))  # arrays: uint64 sums wrap silently, as meant here
    hi = b.sum(dtype=U, keepdims=True) ^ R.fmix64(U((G << 1) | 1))
    return int(lo[0]), int(hi[0])


@pytest.mark.parametrize("B", C.BOUNDS)
def test_sig_ref_equals_numpy_restatement_po(B):
    call = C.po_call(B)
    assert C.bound_of(call) == B  # top_id sets the call's bound
    for p in call:
        assert C.reference(p) == np_signature(p.sym, p.ent), p


def test_sig_ref_equals_numpy_restatement_exact_and_bounded():
    for p in C.exact_call():
        assert C.reference(p) == np_signature(p.sym, None), p
    for p in C.po_call(11, long=False):
        assert C.reference(p, 7) == np_signature(p.sym, p.ent, 7), p
    vals = [0, 1, 2**32 - 1, 2**32, 2**63, 2**64 - 1, 0x0123456789ABCDEF]
    assert [sig_ref.fmix64(v) for v in vals] == R.fmix64(np.array(vals, U)).tolist()
    ranks = [0, 1, 65535, 65536, 65537, 2**31, 2**32 - 1]
    ka, kb = R.rank_keys(np.array(ranks, U))
    assert [sig_ref.rank_key_a(r) for r in ranks] == ka.tolist()
    assert [sig_ref.rank_key_b(r) for r in ranks] == kb.tolist()


def test_probe_set_is_as_stated():
    pool = C.pool().tolist()
    assert 0 in pool and C.M64 in pool and len(set(pool)) == 64
    tails = set()
    for B in C.BOUNDS:
        call = C.po_call(B)
        tails.add(len(call) % 4)
        used = set(np.concatenate([p.sym for p in call]).tolist())
        assert 0 in used and C.M64 in used
        lens = {}
        for p in call:
            lens.setdefault(p.name.split("[")[0], set()).add(len(p))
        for pat in C.PATTERNS:
            want = set(C.SHORT) | (set(C.LONG) if pat in C.LONG_PATTERNS else set())
            assert lens[pat] == want or (pat == "random" and len(want - lens[pat]) <= 3)
        # neighbours in the call differ in length: a workgroup's four waves are not alike
        n = [len(p) for p in call]
        assert sum(1 for k in range(0, len(n) - 3, 4) if len(set(n[k:k + 4])) >= 3) >= len(n) // 4 * 3 // 4
        assert any(0 in n[k:k + 4] and max(n[k:k + 4]) >= 255 for k in range(0, len(n), 4))
    assert tails == {1, 2, 3}
    assert len(C.exact_call()) % 4 != 0
    assert {len(p) for p in C.exact_call()} == set(C.SHORT) | set(C.LONG)
    assert C.po_call(7) == C.po_call(7) and C.probe("random", 513, 65).ent.tolist() == \
        C.entities("random", 513, 65).tolist()


def test_po_probes_are_not_vacuous():
    """From the probe set alone: most steps mix entities and repeat one of them inside the step (both the group
    intersection and the rank inside a group matter), ranks pass the key table, and the two extreme steps exist."""
    one_entity_step = all_distinct_step = False
    for B in C.BOUNDS:
        steps = [s for p in C.po_call(B) if len(p) not in C.LONG for s in C.step_profile(p)]
        assert 51 * len(C.PATTERNS) - 48 <= len(steps) <= 51 * len(C.PATTERNS)  # less up to 3 trimmed probes' steps
        mixed = sum(1 for _taken, distinct, largest in steps if distinct >= 2 and largest >= 2)
        if B >= 7:
            assert 2 * mixed >= len(steps), (B, mixed, len(steps))
        one_entity_step |= any(t == 64 and d == 1 for t, d, _ in steps)
        all_distinct_step |= any(d == 64 for _, d, _ in steps)
    assert one_entity_step and all_distinct_step
    top_rank = max(r for p in C.po_call(64) for r in sig_ref.ranks(len(p), p.ent) if r is not None)
    assert top_rank >= 65536
    assert max(len(p) for p in C.exact_call()) - 1 >= 65536
    # and a long trace whose ranks stay inside the table, as the contrast
    alt2 = [p for p in C.po_call(64) if p.name.startswith("alt2[70000]")][0]
    assert max(sig_ref.ranks(len(alt2), alt2.ent)) < 65536


def _pairs_equal_by_loops(traces, curve):
    """eq[i][j] from the literal loops, one pair at a time."""
    n = len(traces)
    return [[curve([traces[i], traces[j]]) == [1, 1] for j in range(n)] for i in range(n)]


def test_sig_ref_equality_is_the_literal_loops_equality():
    raw = C.short_probes()
    assert len(raw) >= 200
    ids = [[C.NONE if e is None else e for e, _ in t] for t in raw]
    syms = [[s for _, s in t] for t in raw]
    po = [sig_ref.signature(s, e) for s, e in zip(syms, ids)]
    ex = [sig_ref.signature(s) for s in syms]
    eq_po = _pairs_equal_by_loops(raw, O.unique_curve_po)
    eq_ex = _pairs_equal_by_loops(syms, O.unique_curve_exact)
    n = len(raw)
    n_po = n_ex = 0
    for i in range(n):
        for j in range(i + 1, n):
            assert (po[i] == po[j]) == eq_po[i][j], (raw[i], raw[j])
            assert (ex[i] == ex[j]) == eq_ex[i][j], (raw[i], raw[j])
            n_po += eq_po[i][j]
            n_ex += eq_ex[i][j]
    # the relation merges and separates in both modes, and PO merges pairs that exact mode separates
    total = n * (n - 1) // 2
    assert 100 <= n_ex < n_po <= total - 1000
    # the curves, through first_equal
    for sigs, curve in ((po, O.unique_curve_po(raw)), (ex, O.unique_curve_exact(syms))):
        fe = sig_ref.first_equal(sigs)
        assert list(np.cumsum([h == i for i, h in enumerate(fe)])) == curve


def test_relabelling_and_skipped_elements():
    empty = sig_ref.signature([])
    assert empty == sig_ref.signature([], []) == np_signature(np.zeros(0, U), np.zeros(0, np.uint32))
    for B in (7, 65):
        rng = np.random.default_rng(B)
        for p in C.po_call(B, long=False):
            perm = rng.permutation(20000)[:B].astype(np.uint32)  # injective, not onto, ids past 16,384 too
            e2 = np.where(p.ent == C.NONE, np.uint32(C.NONE), perm[np.minimum(p.ent, B - 1)])
            assert sig_ref.signature(p.sym, e2) == C.reference(p), p
            if p.name.startswith("all_none"):
                assert C.reference(p) == empty
            # a bound at or below every id skips everything
            assert sig_ref.signature(p.sym, p.ent, 0) == empty
    p = C.probe("top_id", 65, 7)
    assert sig_ref.signature(p.sym, p.ent, 6) == sig_ref.signature(p.sym[1::2], p.ent[1::2])
    # a merge of two ids is not a relabelling: the signature moves
    q = C.probe("alt2", 65, 7)
    assert sig_ref.signature(q.sym, np.zeros(65, np.uint32)) != C.reference(q)


def test_class_rule_restatement():
    fe = sig_ref.first_equal([(1, 2), (1, 3), (1, 2), (0, 2), (1, 3), (1, 2)])
    assert fe == [0, 1, 0, 3, 1, 0] and sig_ref.n_classes(fe) == 3
    # largest gap, ties to the smallest index, NMZ_NONE off the heads
    assert sig_ref.class_rep(fe, [7, 0, 9, 5, 0, 9]) == [2, 1, C.NONE, 3, C.NONE, C.NONE]
    assert sig_ref.class_rep(fe, [sig_ref.INT64_MAX, 1, 9, 5, 2, sig_ref.INT64_MAX])[:2] == [0, 4]


def test_crafted_class_inputs_are_not_vacuous():
    for fam, N in C.CLASS_CASES:
        sigs = C.class_sigs(fam, N)
        assert len(sigs) == N and all(0 <= lo <= C.M64 and 0 <= hi <= C.M64 for lo, hi in sigs)
        assert C.class_sigs(fam, N) == sigs
        hi_only, lo_only, both = C.pair_agreement(sigs)
        classes = sig_ref.n_classes(sig_ref.first_equal(sigs))
        if fam == "equal":
            assert classes == 1
        elif fam == "distinct":
            assert classes == N
            if N >= 255:  # either half alone would merge thousands of pairs
                assert hi_only >= 1000 and lo_only >= 1000 and both == 0
        elif fam == "grid" and N == 5000:
            # the family the low-half gather is meant to stress
            assert hi_only >= 1000 and lo_only >= 1000 and both >= 1000
            assert classes == 64
        elif fam == "grid" and N >= 255:
            assert hi_only >= 1000 and lo_only >= 1000 and both >= 100
        elif fam == "single_bit":
            assert classes == 129 and both == 129
            vals = sorted({lo | hi << 64 for lo, hi in sigs})
            assert vals == [0] + [1 << b for b in range(128)]
        gaps = C.class_gaps(fam, N)
        assert set(gaps) <= set(C.GAPS)
        if N >= 63:
            assert set(gaps) == set(C.GAPS)
    g = set(C.GRID)
    assert len(g) == 8 and {0, C.M64} <= g
    assert sum(1 for a in g for b in g if a ^ b == 1) >= 4 and sum(1 for a in g for b in g if a ^ b == 1 << 63) >= 4
    # ties for the class representative are frequent
    fe = sig_ref.first_equal(C.class_sigs("grid", 5000))
    gaps = C.class_gaps("grid", 5000)
    best = {}
    for i, h in enumerate(fe):
        best.setdefault(h, []).append(gaps[i])
    assert all(v.count(max(v)) >= 2 for v in best.values())


def test_decreasing_offsets_are_refused_without_a_device():
    """A decreasing pair would wrap n = off[t + 1] - off[t] in the kernel: both host entry points refuse it, and the
    argument checks come before the context check, so the refusal needs no device."""
    L = _lib.load()
    sym = np.arange(8, dtype=U)
    out = np.zeros(8, U)
    bad = np.array([0, 5, 3, 8], U)
    good = np.array([0, 3, 5, 8], U)
    for fn in (L.nmz_trace_signatures, L.nmz_unique_traces):
        assert fn(None, _lib.ptr(bad), _lib.ptr(sym), None, 3, _lib.ptr(out)) == _lib.NMZ_EINVAL
        assert "offsets must be non-decreasing" in _lib.last_error()
        assert fn(None, _lib.ptr(good), _lib.ptr(sym), None, 3, _lib.ptr(out)) == _lib.NMZ_EINVAL
        assert "ctx is NULL" in _lib.last_error()
        assert fn(None, None, _lib.ptr(sym), None, 3, _lib.ptr(out)) == _lib.NMZ_EINVAL
        assert "NULL argument" in _lib.last_error()
        assert fn(None, _lib.ptr(good), None, None, 3, _lib.ptr(out)) == _lib.NMZ_EINVAL
        assert "sym is NULL" in _lib.last_error()
        # the last pair decreasing, and a first offset above the second
        for off in ([0, 3, 8, 7], [4, 3, 5, 8]):
            assert fn(None, _lib.ptr(np.array(off, U)), _lib.ptr(sym), None, 3, _lib.ptr(out)) == _lib.NMZ_EINVAL
            assert "offsets must be non-decreasing" in _lib.last_error()
        assert fn(None, None, None, None, 0, None) == _lib.NMZ_EINVAL
        assert "ctx is NULL" in _lib.last_error()
