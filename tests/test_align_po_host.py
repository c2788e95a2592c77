"""CPU: edit scripts per entity on the host (nmz_ed_align_po_host) against the definition.

tests/po_ref.py is DESIGN.md section 2, "Edit scripts per entity", in pure Python over tests/align_ref.py. The host
form is tied to it op for op, to the answers known by hand, to nmz_ed_align_wide_host's bytes with one entity, and to
the oracle's literal tracesEqualInPO loop (dist == 0). tests/test_align_po_gpu.py takes its expected values from this
host form; the counts that keep its family from being vacuous are asserted here, from the host form alone. Every
comparison is integer equality, slot for slot."""
import ctypes
import functools

import numpy as np
import pytest

import align_ref as AR
import ed_cases as EC
import po_ref as PR
from namazu_amd import _lib
from namazu_amd import historystorage as hs
from oracle import oracle as O
from test_align_wide_host import wide_slots

NONE = _lib.NMZ_NONE
NONE3 = (NONE,) * 3
S, D, I = AR.SUB, AR.DEL, AR.INS
SPARSE = {0: 0, 1: 5, 2: 37, 3: NONE}
MAPS = {"mod2": (lambda v: v % 2, 2), "sparse": (lambda v: SPARSE[v], 38), "one": (lambda v: 0, 1)}
BANDS = (8, 32, 64, 65, 128, 256, 1024)


def ent_of(ids, name):
    """entity[len(ids)] (uint32) of dense symbol ids under the map `name`, and its n_entities."""
    f, G = MAPS[name]
    return np.array([f(int(v)) for v in ids], np.uint32), G


def po_slots(a, ea, b, eb, G, w):
    """(dist, ops[w]) of nmz_ed_align_po_host: all `band` slots, sentinels included."""
    a, b = np.ascontiguousarray(a, np.uint64), np.ascontiguousarray(b, np.uint64)
    ea, eb = np.ascontiguousarray(ea, np.uint32), np.ascontiguousarray(eb, np.uint32)
    dist = ctypes.c_uint32()
    ops = np.zeros(w, _lib.EDIT_OP_DTYPE)
    _lib.check(_lib.load().nmz_ed_align_po_host(_lib.ptr(a), _lib.ptr(ea), len(a), _lib.ptr(b), _lib.ptr(eb), len(b), G,
                                                w, ctypes.byref(dist), _lib.ptr(ops) if w else None))
    return dist.value, ops


def po(a, ea, b, eb, w, G=None):
    d, sc = hs.edit_script_po_host(a, ea, b, eb, w, n_entities=G)
    return d, (None if sc is None else AR.as_tuples(sc))


# ---- 1. the answers known by hand ------------------------------------------------------------------------------------
def rot(k):
    """X^k B -> B X^k, the rotation row of tests/moves_wide_cases.py: X = 1, B a block of 3 k distinct symbols.
    Returns a, b and their entities with X in entity 0 and B in entity 1."""
    blk = list(range(10, 10 + 3 * k))
    return [1] * k + blk, blk + [1] * k, [0] * k + [1] * 3 * k, [1] * 3 * k + [0] * k


def test_hand_table():
    x1, y1, x2, y2, a_, b_, c_, p_, q_ = range(10, 19)
    rows = [
        ([x1, y1, x2, y2], [0, 1, 0, 1], [y1, y2, x1, x2], [1, 1, 0, 0], 4, 4, 0, []),
        ([a_, b_, c_], [0, 1, 0], [a_, c_], [0, 0], 2, 1, 1, [(1, 2, D)]),
        ([a_, c_], [0, 0], [a_, b_, c_], [0, 1, 0], 2, 1, 1, [(2, 1, I)]),
        ([p_, q_], [0, 1], [q_, p_], [1, 0], 2, 2, 0, []),
        ([p_], [0], [q_], [1], 2, 1, 2, [(0, 1, D), (1, 0, I)]),
    ]
    for a, ea, b, eb, w, exact, dist, sc in rows:
        assert wide_slots(a, b, w)[0] == exact
        assert PR.script(a, ea, b, eb, w) == (dist, sc)
        assert po(a, ea, b, eb, w) == (dist, sc), (a, b)
        d, ops = po_slots(a, ea, b, eb, 2, w)
        assert d == dist and AR.as_tuples(ops[dist:]) == [NONE3] * (w - dist)
    for k in (3, 33):
        a, b, split_a, split_b = rot(k)
        assert wide_slots(a, b, 2 * k)[0] == 2 * k
        assert po(a, split_a, b, split_b, 2 * k) == (0, [])
        d1, o1 = po_slots(a, [0] * 4 * k, b, [0] * 4 * k, 1, 2 * k)
        dw, ow = wide_slots(a, b, 2 * k)
        assert d1 == dw == 2 * k and o1.tobytes() == ow.tobytes()
        assert po(a, [0] * 4 * k, b, [0] * 4 * k, 2 * k - 1) == (2 * k, None)


# ---- 2. the definition ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def small_family():
    """10 traces over {0, 1, 2, 3}, lengths 0 .. 40: two bases, each plain, lightly and heavily edited, a rotation,
    the empty trace and a single element."""
    rng = np.random.default_rng(410)
    out = [np.zeros(0, np.int64), np.array([2], np.int64)]
    for L in (17, 38):
        base = rng.integers(0, 4, size=L).astype(np.int64)
        out += [base, EC._edited(base, 3, 4, rng)[:40], EC._edited(base, 9, 4, rng)[:40], np.roll(base, 5)]
    return tuple(out)


@pytest.mark.parametrize("name", sorted(MAPS))
def test_po_host_equals_definition(name):
    trs = small_family()
    ents = [ent_of(t, name)[0] for t in trs]
    G = MAPS[name][1]
    within = beyond = 0
    for w in range(13):
        for i, j in EC.all_ordered_pairs(len(trs)).tolist():
            want = PR.script(trs[i].tolist(), ents[i].tolist(), trs[j].tolist(), ents[j].tolist(), w)
            assert po(trs[i], ents[i], trs[j], ents[j], w, G) == want, (name, w, i, j)
            d, ops = po_slots(trs[i], ents[i], trs[j], ents[j], G, w)
            k = d if d <= w else 0
            assert d == want[0] and AR.as_tuples(ops[k:]) == [NONE3] * (w - k)
            within += d <= w and d > 0
            beyond += d > w
    assert within >= 100 and beyond >= 100


def test_one_entity_equals_the_wide_host_form():
    trs = small_family()
    for w in (0, 3, 12, 65):
        for i, j in EC.all_ordered_pairs(len(trs)).tolist():
            e_i, e_j = np.zeros(len(trs[i]), np.uint32), np.zeros(len(trs[j]), np.uint32)
            d, ops = po_slots(trs[i], e_i, trs[j], e_j, 1, w)
            dw, ow = wide_slots(trs[i], trs[j], w)
            assert d == dw and ops.tobytes() == ow.tobytes()


def test_script_by_entity_splits_the_segments():
    trs = small_family()
    a, b = trs[7], trs[8]
    ea, eb = ent_of(a, "sparse")[0], ent_of(b, "sparse")[0]
    d, sc = hs.edit_script_po_host(a, ea, b, eb, 40, n_entities=38)
    assert 0 < d <= 40
    seg = hs.script_by_entity(ea, eb, sc)
    assert list(seg) == sorted(seg) and set(seg) <= {0, 5, 37} and sum(len(v) for v in seg.values()) == d
    assert np.concatenate([seg[g] for g in seg]).tobytes() == sc.tobytes()


# ---- 3. dist == 0 <=> tracesEqualInPO -----------------------------------------------------------------------------------
def interleavings(rng, n, n_perturbed, lens=(7, 9, 5)):
    """n random interleavings of fixed per-entity sequences (entity g's symbols are 100 g + 0 .. 3), plus n_perturbed
    with one element changed to another symbol of its entity. Returns [(symbols, entities)]."""
    seqs = [[100 * g + int(x) for x in rng.integers(0, 4, size=L)] for g, L in enumerate(lens)]
    out = []
    for r in range(n + n_perturbed):
        order = rng.permutation(np.repeat(np.arange(len(lens)), lens))
        at = [0] * len(lens)
        sym = []
        for g in order:
            sym.append(seqs[g][at[g]])
            at[g] += 1
        if r >= n:
            p = int(rng.integers(0, len(sym)))
            sym[p] = 100 * (sym[p] // 100) + (sym[p] % 100 + 1) % 4
        out.append((np.array(sym, np.uint64), order.astype(np.uint32)))
    return out


def test_dist_zero_iff_equal_in_po():
    rng = np.random.default_rng(62)
    trs = interleavings(rng, 10, 6)
    zero = nonzero = 0
    for i, (a, ea) in enumerate(trs):
        for j, (b, eb) in enumerate(trs):
            same = O.unique_curve_po([list(zip(ea.tolist(), a.tolist())), list(zip(eb.tolist(), b.tolist()))]) == [1, 1]
            assert same == PR.equal_in_po(a.tolist(), ea.tolist(), b.tolist(), eb.tolist())
            d, sc = po(a, ea, b, eb, 30, 3)
            assert (d == 0) == same and (sc == []) == same
            zero += same and i != j
            nonzero += not same
    assert zero >= 40 and nonzero >= 40


# ---- 4. limits: each refusal with its message and no device -------------------------------------------------------------
def test_po_host_refusals():
    L = _lib.load()
    a, b = np.arange(3, dtype=np.uint64), np.arange(1, 4, dtype=np.uint64)
    e = np.array([0, 1, NONE], np.uint32)
    bad = np.array([0, 2, NONE], np.uint32)
    dist = ctypes.c_uint32()
    ops = np.zeros(1025, _lib.EDIT_OP_DTYPE)
    P = _lib.ptr

    def call(a=P(a), ea=P(e), n=3, b=P(b), eb=P(e), m=3, G=2, band=70, dist=ctypes.byref(dist), ops=P(ops)):
        return L.nmz_ed_align_po_host(a, ea, n, b, eb, m, G, band, dist, ops)

    for kw, msg in [
        ({"band": 1025}, "band 1025 exceeds NMZ_ALIGN_WIDE_MAX_BAND (1024)"),
        ({"n": 2**32 - 1}, "a has 4294967295 elements"),
        ({"m": 2**32 - 1}, "b has 4294967295 elements"),
        ({"a": None}, "a or b is NULL"),
        ({"dist": None}, "dist is NULL"),
        ({"ops": None}, "ops is NULL"),
        ({"ea": None}, "entity is NULL"),
        ({"eb": None}, "entity is NULL"),
        ({"G": 0}, "n_entities 0 must be 1 .. NMZ_PO_MAX_ENTITIES (1024)"),
        ({"G": 1025}, "n_entities 1025 must be 1 .. NMZ_PO_MAX_ENTITIES (1024)"),
        ({"ea": P(bad)}, "a's element 1 has entity id 2: ids are < n_entities (2) or NMZ_NONE"),
        ({"eb": P(bad)}, "b's element 1 has entity id 2: ids are < n_entities (2) or NMZ_NONE"),
    ]:
        assert call(**kw) == _lib.NMZ_EINVAL, kw
        assert msg in _lib.last_error(), (kw, _lib.last_error())
    assert call(G=1024) == _lib.NMZ_OK
    assert L.nmz_ed_align_po_host(None, None, 0, None, None, 0, 1, 0, ctypes.byref(dist), None) == _lib.NMZ_OK
    assert dist.value == 0 and _lib.NMZ_PO_MAX_ENTITIES == 1024


def test_po_pairs_refusals_need_no_device():
    """Every limit of nmz_ed_align_po_pairs, nmz_ed_diff_profile_po, nmz_po_project and of the plan is checked before
    the context (ctx = NULL): the aligner's own first, with its messages, then the entities."""
    L = _lib.load()
    P = _lib.ptr
    sym = np.arange(8, dtype=np.uint64)
    off = np.array([0, 3, 3, 8], np.uint64)
    ent = np.array([0, 1, NONE, 1, 1, 0, 3, 2], np.uint32)
    pairs = np.array([[0, 2], [1, 1]], np.uint32)
    dist = np.zeros(2, np.uint32)
    ops = np.zeros((2, 1024), _lib.EDIT_OP_DTYPE)
    usym = sym.copy()
    counts = np.zeros(8, _lib.MOVE_COUNTS_DTYPE)
    info = np.zeros(1, _lib.MOVE_INFO_DTYPE)

    def pairs_call(off=off, sym=sym, ent=ent, n_traces=3, G=4, pairs=pairs, n_pairs=2, band=100, dist=dist, ops=ops):
        return L.nmz_ed_align_po_pairs(None, P(off), P(sym), P(ent), n_traces, G, P(pairs), n_pairs, band, P(dist),
                                       P(ops))

    def prof_call(off=off, sym=sym, ent=ent, n_traces=3, G=4, pairs=pairs, n_pairs=2, band=100, dist=dist, ops=None):
        return L.nmz_ed_diff_profile_po(None, P(off), P(sym), P(ent), n_traces, G, P(pairs), n_pairs, band, P(usym), 8,
                                        P(dist), P(counts), P(info))

    shared = [
        ({}, "ctx is NULL"),
        ({"band": 8}, "ctx is NULL"),
        ({"band": 1024, "G": 1024}, "ctx is NULL"),
        ({"band": 1025}, "band 1025 exceeds NMZ_ALIGN_WIDE_MAX_BAND (1024)"),
        ({"pairs": np.array([[0, 3], [1, 1]], np.uint32)}, "pair index out of range (pair 0)"),
        ({"off": np.array([0, 5, 3, 8], np.uint64)}, "offsets must be non-decreasing (trace 1)"),
        ({"off": np.array([0, 2**32 - 1, 2**32, 2**32], np.uint64)}, "trace 0 has 4294967295 elements"),
        ({"sym": None}, "sym is NULL"),
        ({"ent": None}, "entity is NULL"),
        ({"G": 0}, "n_entities 0 must be 1 .. NMZ_PO_MAX_ENTITIES (1024)"),
        ({"G": 1025}, "n_entities 1025 must be 1 .. NMZ_PO_MAX_ENTITIES (1024)"),
        ({"G": 3}, "element 6 has entity id 3: ids are < n_entities (3) or NMZ_NONE"),
        ({"pairs": np.array([[0, 3], [1, 1]], np.uint32), "G": 3}, "pair index out of range (pair 0)"),  # the order
    ]
    for call in (pairs_call, prof_call):
        for kw, msg in shared:
            assert call(**kw) == _lib.NMZ_EINVAL, kw
            assert msg in _lib.last_error(), (kw, _lib.last_error())
    for kw, msg in [({"off": None}, "off, pairs or dist is NULL"), ({"pairs": None}, "off, pairs or dist is NULL"),
                    ({"dist": None}, "off, pairs or dist is NULL"), ({"ops": None}, "ops is NULL")]:
        assert pairs_call(**kw) == _lib.NMZ_EINVAL, kw
        assert msg in _lib.last_error(), (kw, _lib.last_error())
    assert pairs_call(n_pairs=0) == _lib.NMZ_OK  # legal, and needs no device
    assert pairs_call(n_pairs=0, band=0, ops=None, dist=None) == _lib.NMZ_OK
    assert pairs_call(n_pairs=0, G=0) == _lib.NMZ_EINVAL and "NMZ_PO_MAX_ENTITIES" in _lib.last_error()
    counts["later"] = 7
    assert prof_call(n_pairs=0) == _lib.NMZ_OK and not counts["later"].any()
    ts = hs.TraceSet([sym[:3], sym[3:]])
    es = hs.edit_scripts_po(ts, ent, np.zeros((0, 2), np.uint32), 300)
    assert es.dist.shape == (0,) and es.ops.shape == (0, 300)
    with pytest.raises(_lib.NmzInvalidArgument, match="NMZ_PO_MAX_ENTITIES"):
        hs.edit_scripts_po(ts, ent, np.array([[0, 1]], np.uint32), 8, n_entities=0)
    with pytest.raises(_lib.NmzInvalidArgument, match="NMZ_PO_MAX_ENTITIES"):
        hs.move_profile_po(ts, ent, np.array([[0, 1]], np.uint32), 8, n_entities=2000)
    # the projection
    poff = np.zeros(3 * 4 + 1, np.uint64)
    psym, psrc = np.zeros(8, np.uint64), np.zeros(8, np.uint32)
    for args, msg in [
        ((None, P(off), P(sym), P(ent), 3, 4, P(poff), P(psym), P(psrc)), "ctx is NULL"),
        ((None, None, P(sym), P(ent), 3, 4, P(poff), P(psym), P(psrc)), "off or poff is NULL"),
        ((None, P(off), None, P(ent), 3, 4, P(poff), P(psym), P(psrc)), "sym is NULL"),
        ((None, P(off), P(sym), None, 3, 4, P(poff), P(psym), P(psrc)), "entity is NULL"),
        ((None, P(off), P(sym), P(ent), 3, 0, P(poff), P(psym), P(psrc)), "NMZ_PO_MAX_ENTITIES (1024)"),
        ((None, P(off), P(sym), P(ent), 3, 3, P(poff), P(psym), P(psrc)), "element 6 has entity id 3"),
        ((None, P(off), P(sym), P(ent), 3, 4, P(poff), None, P(psrc)), "psym or psrc is NULL"),
    ]:
        assert L.nmz_po_project(*args) == _lib.NMZ_EINVAL, msg
        assert msg in _lib.last_error(), (msg, _lib.last_error())
    poff[0] = 9
    assert L.nmz_po_project(None, P(off), None, None, 0, 4, P(poff), None, None) == _lib.NMZ_OK and poff[0] == 0
    # the plan and the device form
    plan = ctypes.c_void_p(1)
    for args, msg in [
        ((None, 1025, 4, 100, 10), "NMZ_ALIGN_WIDE_MAX_BAND (1024)"),
        ((None, 100, 0, 100, 10), "NMZ_PO_MAX_ENTITIES (1024)"),
        ((None, 100, 1025, 100, 10), "NMZ_PO_MAX_ENTITIES (1024)"),
        ((None, 100, 4, 100, 0), "max_pairs is 0"),
        ((None, 100, 4, 2**32 - 1, 10), "a trace of max_len has 4294967295 elements"),
        ((None, 100, 4, 100, 10), "ctx is NULL"),
    ]:
        assert L.nmz_ed_align_po_plan_create(*args, ctypes.byref(plan)) == _lib.NMZ_EINVAL, msg
        assert msg in _lib.last_error() and plan.value is None, (msg, _lib.last_error())
        plan = ctypes.c_void_p(1)
    assert L.nmz_ed_align_po_plan_destroy(None) == _lib.NMZ_OK
    assert L.nmz_ed_align_po_pairs_dev(None, None, None, None, None, None, 0, None, None, None) == _lib.NMZ_EINVAL
    assert "plan is NULL" in _lib.last_error()


# ---- 5. the GPU family is not vacuous -----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def gpu_family(name):
    """tests/test_align_wide_gpu.py's family with the entities of map `name`: (traces, entities, n_entities)."""
    from test_align_wide_gpu import family
    ids = {int(EC.encode([v])[0]): v for v in range(4)}
    trs = family()
    ents = tuple(ent_of([ids[int(x)] for x in t], name)[0] for t in trs)
    return trs, ents, MAPS[name][1]


_memo = {}


def expected(name, pairs, w):
    """dist[P], ops[P][w] of nmz_ed_align_po_host over the GPU family, computed once per (map, band, pair)."""
    trs, ents, G = gpu_family(name)
    dist = np.zeros(len(pairs), np.uint32)
    ops = np.zeros((len(pairs), w), _lib.EDIT_OP_DTYPE)
    for p, (i, j) in enumerate(np.asarray(pairs).tolist()):
        key = (name, w, i, j)
        if key not in _memo:
            _memo[key] = po_slots(trs[i], ents[i], trs[j], ents[j], G, w)
        dist[p], ops[p] = _memo[key]
    return dist, ops


@pytest.mark.parametrize("name", ["mod2", "sparse"])
def test_gpu_family_is_not_vacuous(name):
    """The PO distance of every ordered pair at band 1,024 from the host form; at a band w it is min(d, w + 1) by
    the definition, and a pair beyond 1,024 is beyond every band. The host form counts, the 42 (i, i) pairs included:
    mod2 138 / 242 / 450 / 512 / 820 / 1,146 / 1,528 pairs within the seven bands, sparse 184 / 270 / 654 / 654 / 880 /
    1,304 / 1,604; at least 160 pairs beyond at every band."""
    trs, ents, G = gpu_family(name)
    pairs = EC.all_ordered_pairs(len(trs))
    d, _ = expected(name, pairs, 1024)
    exact = np.array([wide_slots(trs[i], trs[j], 1024)[0] for i, j in pairs.tolist()], np.uint32)
    for w in BANDS:
        within, beyond = int((d <= w).sum()), int((d > w).sum())
        mid = int(((d > 64) & (d <= w)).sum())
        print(name, w, "within", within, "beyond", beyond, "within and > 64", mid)
        assert within >= 16 and beyond >= 16
        if w in (128, 256, 1024):
            assert mid >= 8
    known = (d <= 1024) | (exact <= 1024)  # at least one side is exact, so the comparison is
    less, more = int((known & (d < exact)).sum()), int((known & (d > exact)).sum())
    print(name, "PO < exact", less, "PO > exact", more)
    assert less >= 8 and more >= 2
