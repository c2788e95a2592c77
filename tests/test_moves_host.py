"""CPU: the move profile's host forms (nmz_script_moves_host, nmz_move_profile_host) against the definition.

tests/moves_ref.py is the definition in pure Python over tests/align_ref.py's scripts; tests/golden/
move_profile_kat.json holds known answers made by a third program (plain scans, no queues). The host forms are tied
to both here, value for value, on the known answers and on a random family whose counts below show that it holds
moves in both directions, values that move twice, unequal DEL / INS counts and scripts as long as the band -- so the
GPU comparison (tests/test_moves_gpu.py, which takes its expected values from the host forms) cannot pass
vacuously."""
import functools

import numpy as np
import pytest

import align_ref as AR
import moves_cases as MC
import moves_ref as MR
from namazu_amd import _lib
from namazu_amd import historystorage as hs

NONE = _lib.NMZ_NONE
BANDS = [8, 31, 63, 64]


def table_of(ids):
    """(usym, id of every table entry) for a set of dense symbol ids: the table is sorted by the encoded value."""
    ids = sorted(ids, key=MC.encode_one)
    return np.array([MC.encode_one(v) for v in ids], np.uint64), ids


def check_profile(prof, ids, counts, info, partner=None):
    """A MoveProfile against moves_ref.profile's (partner, counts, info): every counter of every table symbol."""
    assert {f: int(prof.info[f]) for f in info} == info
    assert len(prof.counts) == len(ids)
    for u, v in enumerate(ids):
        got = {f: int(prof.counts[u][f]) for f in MR.FIELDS}
        assert got == counts.get(v, MR.empty_counts()), (v, got)
    if partner is not None:
        want = np.array([[NONE if q is None else q for q in row] for row in partner], np.uint32)
        want = want.reshape(prof.partner.shape)
        assert np.array_equal(prof.partner, want), np.nonzero((prof.partner != want).any(axis=1))[0][:10]


@functools.lru_cache(maxsize=None)
def family_ref(w):
    """(traces, pairs, moves_ref.profile over them, {(i, j): (dist, ops)}) of the random family at band w."""
    fam = MC.family(w)
    pairs = MC.ordered_pairs(len(fam))
    scripts = {(i, j): AR.script(fam[i], fam[j], w, band=w) for i, j in pairs}
    return fam, pairs, MR.profile(fam, pairs, w, scripts=scripts), scripts


# ---- 1. the fixture -------------------------------------------------------------------------------------------------
def test_known_answers(golden):
    kat = golden("move_profile_kat.json")
    names = {c["name"] for c in kat}
    assert {"abab-baba", "abcde-bcdex", "ab-ba", "kitten-sitting", "rot32-w64", "rot32-w64-rev", "rot31-w63",
            "rot16-w32", "rot15-w31", "xy16-w64", "x34-x30-w64", "x30-x34-w64"} <= names
    for c in kat:
        a, b, w = c["a"], c["b"], c["band"]
        dist, ops = AR.script(a, b, w, band=w)
        assert dist == c["dist"] and (ops is None) == (c["ops"] is None), c["name"]
        want_counts = {int(v): dict(rec, reserved=0) for v, rec in c["counts"].items()}
        partner, counts, info, _ = MR.profile([a, b], [(0, 1)], w)
        assert counts == want_counts and info == c["info"], c["name"]
        ea, eb = MC.encode(a), MC.encode(b)
        usym, ids = table_of(set(a) | set(b))
        es = MC.host_scripts([ea, eb], [(0, 1)], w)
        prof = hs.move_profile_of(hs.TraceSet([ea, eb]), [[0, 1]], es, usym=usym, want_partner=True, host=True)
        assert int(prof.dist[0]) == dist
        if ops is None:
            assert (prof.partner == NONE).all()
            check_profile(prof, ids, {}, c["info"])
            continue
        assert [tuple(o) for o in c["ops"]] == ops == AR.as_tuples(es.script(0))
        assert partner[0][:dist] == c["partner"] == MR.partners(a, b, ops)
        check_profile(prof, ids, want_counts, c["info"], partner)
        got = hs.script_partners(ea, eb, es.script(0))
        assert [None if q == NONE else int(q) for q in got] == c["partner"]
    by = {c["name"]: c for c in kat}
    assert by["rot32-w64"]["partner"][31] == 63 and by["rot32-w64"]["partner"][63] == 31  # 32 lanes apart
    assert by["abab-baba"]["counts"][str(ord("b"))]["span_earlier"] == 4


# ---- 2. the host forms on the random family ----------------------------------------------------------------------------
@pytest.mark.parametrize("w", BANDS)
def test_host_profile_equals_definition(w):
    fam, pairs, (partner, counts, info, dist), _ = family_ref(w)
    trs = [MC.encode(t) for t in fam]
    usym, ids = table_of({x for t in fam for x in t})
    es = MC.host_scripts(trs, pairs, w)
    assert es.dist.tolist() == dist
    prof = hs.move_profile_of(hs.TraceSet(trs), pairs, es, usym=usym, want_partner=True, host=True)
    check_profile(prof, ids, counts, info, partner)
    assert info["n_unknown"] == 0 and info["n_scripts"] + info["n_beyond"] == len(pairs) == 870
    # partner == NULL: the same counters
    plain = hs.move_profile_of(hs.TraceSet(trs), pairs, es, usym=usym, host=True)
    assert plain.partner is None and plain.counts.tobytes() == prof.counts.tobytes() and plain.info == prof.info


@pytest.mark.parametrize("w", BANDS)
def test_script_partners_equal_script_moves(w):
    """nmz_script_moves_host against the definition and against script_moves, move for move."""
    fam, pairs, _, scripts = family_ref(w)
    n_moves = 0
    for i, j in pairs:
        d, ops = scripts[(i, j)]
        if not ops:
            continue
        a, b = MC.encode(fam[i]), MC.encode(fam[j])
        sc = np.array(ops, np.uint32).view(_lib.EDIT_OP_DTYPE).reshape(-1)
        pr = hs.script_partners(a, b, sc)
        assert [None if q == NONE else int(q) for q in pr] == MR.partners(fam[i], fam[j], ops)
        mv = sorted((int(a[sc[s]["a_pos"]]), int(sc[s]["a_pos"]), int(sc[int(pr[s])]["b_pos"]))
                    for s in range(d) if sc[s]["kind"] == AR.DEL and pr[s] != NONE)
        assert sorted(mv, key=lambda t: (t[1], t[2])) == hs.script_moves(a, b, sc)
        n_moves += len(mv)
    assert n_moves >= 40


# ---- 3. non-vacuity, from moves_ref alone --------------------------------------------------------------------------
@pytest.mark.parametrize("w", BANDS)
def test_family_exercises_the_rule(w):
    fam, pairs, _, scripts = family_ref(w)
    later = earlier = both = twice = unequal = full = 0
    for i, j in pairs:
        d, ops = scripts[(i, j)]
        if ops is None:
            continue
        lt, el, tw, un = MR.script_kinds(fam[i], fam[j], ops)
        later, earlier, both = later + lt, earlier + el, both + (lt and el)
        twice, unequal, full = twice + tw, unequal + un, full + (d == w)
    print(w, dict(later=later, earlier=earlier, both=both, twice=twice, unequal=unequal, full=full))
    if w == 8:
        assert later >= 15 and earlier >= 15
    else:
        assert later >= 50 and earlier >= 50 and both >= 20 and twice >= 12 and unequal >= 25
    if w == 64:
        assert full >= 50


# ---- 4. the table: a missing symbol, an empty table ------------------------------------------------------------------
def test_table_without_one_symbol_and_empty_table():
    w = 31
    fam, pairs, (partner, counts, info, _), scripts = family_ref(w)
    trs = [MC.encode(t) for t in fam]
    ts = hs.TraceSet(trs)
    es = MC.host_scripts(trs, pairs, w)
    gone = max(counts, key=lambda v: counts[v]["n_pairs"])
    _, c2, i2, _ = MR.profile(fam, pairs, w, table={0, 1, 2, 3} - {gone}, scripts=scripts)
    all_names = [v for (i, j), (_, ops) in scripts.items() if ops for op in ops for v in MR.names(fam[i], fam[j], op)
                 if v is not None]
    named = len(all_names)
    assert i2["n_unknown"] == all_names.count(gone) > 0 and gone not in c2
    usym, ids = table_of({0, 1, 2, 3} - {gone})
    prof = hs.move_profile_of(ts, pairs, es, usym=usym, want_partner=True, host=True)
    check_profile(prof, ids, c2, i2, partner)  # the partners are those of the full table
    empty = hs.move_profile_of(ts, pairs, es, usym=np.zeros(0, np.uint64), want_partner=True, host=True)
    assert len(empty.counts) == 0 and int(empty.info["n_unknown"]) == named
    check_profile(empty, [], {}, dict(info, n_unknown=named), partner)


# ---- 5. refusals and edges ---------------------------------------------------------------------------------------------
def _small():
    sym = np.arange(8, dtype=np.uint64)
    off = np.array([0, 3, 3, 8], np.uint64)
    pairs = np.array([[0, 2], [1, 1]], np.uint32)
    dist = np.array([2, 0], np.uint32)
    ops = np.zeros((2, 8), _lib.EDIT_OP_DTYPE)
    ops[:] = (NONE, NONE, NONE)
    ops[0, 0] = (0, 0, AR.DEL)
    ops[0, 1] = (3, 4, AR.INS)
    return sym, off, pairs, dist, ops


def test_profile_refusals_need_no_device():
    """Every limit of the host-pointer forms is checked before the context: a NULL context never gets that far."""
    L = _lib.load()
    sym, off, pairs, dist, ops = _small()
    usym = np.arange(8, dtype=np.uint64)
    counts = np.zeros(8, _lib.MOVE_COUNTS_DTYPE)
    info = np.zeros(1, _lib.MOVE_INFO_DTYPE)
    partner = np.zeros((2, 8), np.uint32)

    def bad_op(slot, op):
        o = ops.copy()
        o[0, slot] = op
        return o

    def forms(off=off, n_traces=3, pairs=pairs, n_pairs=2, band=8, dist=dist, ops=ops, usym=usym, n_usym=8,
              counts=counts, info=info, only=None):
        given = (_lib.ptr(off), _lib.ptr(sym), n_traces, _lib.ptr(pairs), n_pairs, band, _lib.ptr(dist), _lib.ptr(ops),
                 _lib.ptr(usym), n_usym, _lib.ptr(partner), _lib.ptr(counts), _lib.ptr(info))
        made = (None, _lib.ptr(off), _lib.ptr(sym), n_traces, _lib.ptr(pairs), n_pairs, band, _lib.ptr(usym), n_usym,
                _lib.ptr(dist), _lib.ptr(counts), _lib.ptr(info))
        out = {"host": lambda: L.nmz_move_profile_host(*given), "given": lambda: L.nmz_move_profile(None, *given),
               "made": lambda: L.nmz_ed_diff_profile(*made)}
        return {k: f for k, f in out.items() if only is None or k in only}

    with_ops = ("host", "given")
    for kw, msg in [
        ({"band": 65}, "wider bands are not built yet"),
        ({"pairs": np.array([[0, 3], [1, 1]], np.uint32)}, "pair index out of range (pair 0)"),
        ({"off": np.array([0, 5, 3, 8], np.uint64)}, "offsets must be non-decreasing (trace 1)"),
        ({"off": np.array([0, 2**32 - 1, 2**32, 2**32], np.uint64)}, "trace 0 has 4294967295 elements"),
        ({"dist": None, "only": with_ops}, "off, pairs or dist is NULL"),
        ({"ops": None, "only": with_ops}, "ops is NULL"),
        ({"usym": None}, "usym or counts is NULL"),
        ({"counts": None}, "usym or counts is NULL"),
        ({"info": None}, "info is NULL"),
        ({"usym": np.array([0, 1, 2, 3, 3, 5, 6, 7], np.uint64)}, "usym must be strictly increasing (entry 4)"),
        ({"usym": np.array([0, 1, 2, 3, 4, 5, 7, 6], np.uint64)}, "usym must be strictly increasing (entry 7)"),
        ({"n_pairs": 2**32 // 8}, "must stay below 2^32"),
        ({"ops": bad_op(1, (3, 4, 3)), "only": with_ops}, "op kind 3 is not SUB, DEL or INS (pair 0, slot 1)"),
        ({"ops": bad_op(0, (3, 0, AR.DEL)), "only": with_ops}, "a_pos 3 is outside a trace of 3 elements (pair 0, slot 0)"),
        ({"ops": bad_op(0, (3, 0, AR.SUB)), "only": with_ops}, "a_pos 3 is outside a trace of 3 elements (pair 0, slot 0)"),
        ({"ops": bad_op(1, (3, 5, AR.INS)), "only": with_ops}, "b_pos 5 is outside a trace of 5 elements (pair 0, slot 1)"),
        ({"ops": bad_op(1, (2, 5, AR.SUB)), "only": with_ops}, "b_pos 5 is outside a trace of 5 elements (pair 0, slot 1)"),
    ]:
        for name, f in forms(**kw).items():
            assert f() == _lib.NMZ_EINVAL, (name, kw)
            assert msg in _lib.last_error(), (name, kw, _lib.last_error())
    # a_pos == n is an INS's to have; slots behind dist and scripts beyond the band are not read
    ok = bad_op(1, (3, 4, AR.INS))
    ok[0, 5] = (99, 99, 7)
    ok[1, 0] = (99, 99, 7)
    assert forms(ops=ok)["host"]() == _lib.NMZ_OK
    beyond = forms(ops=bad_op(0, (99, 99, 7)), dist=np.array([9, 0], np.uint32))
    assert beyond["host"]() == _lib.NMZ_OK and int(info[0]["n_beyond"]) == 1 and int(info[0]["n_scripts"]) == 1
    # with valid arguments the device forms get as far as the context
    for name in ("given", "made"):
        assert forms()[name]() == _lib.NMZ_EINVAL and "ctx is NULL" in _lib.last_error()
    assert L.nmz_move_profile_dev(None, None, None, None, 0, 8, None, None, None, 0, None, None, None, 0, None) \
        == _lib.NMZ_EINVAL and "ctx is NULL" in _lib.last_error()


def test_no_pairs_need_no_device():
    L = _lib.load()
    sym, off, pairs, dist, ops = _small()
    usym = np.arange(8, dtype=np.uint64)
    for form in ("host", "given", "made"):
        counts = np.full(8 * 12, 7, np.uint32).view(_lib.MOVE_COUNTS_DTYPE)
        info = np.full(8, 7, np.uint32).view(_lib.MOVE_INFO_DTYPE)
        if form == "made":
            rc = L.nmz_ed_diff_profile(None, _lib.ptr(off), _lib.ptr(sym), 3, _lib.ptr(pairs), 0, 8, _lib.ptr(usym), 8,
                                       None, _lib.ptr(counts), _lib.ptr(info))
        else:
            f = L.nmz_move_profile_host if form == "host" else (lambda *a: L.nmz_move_profile(None, *a))
            rc = f(_lib.ptr(off), _lib.ptr(sym), 3, _lib.ptr(pairs), 0, 8, _lib.ptr(dist), _lib.ptr(ops), _lib.ptr(usym),
                   8, None, _lib.ptr(counts), _lib.ptr(info))
        assert rc == _lib.NMZ_OK, (form, _lib.last_error())
        assert not counts.view(np.uint32).any() and not info.view(np.uint32).any()
    ts = hs.TraceSet([sym[:3], sym[3:]])
    prof = hs.move_profile(ts, np.zeros((0, 2), np.uint32), 8)  # no context is made for it
    assert prof.symbols.tolist() == list(range(8)) and not prof.counts.view(np.uint32).any() and prof.top(3) == []
    assert prof.dist.shape == (0,) and int(prof.info["n_scripts"]) == 0
    with pytest.raises(_lib.NmzInvalidArgument, match="wider bands are not built yet"):
        hs.move_profile(ts, np.zeros((0, 2), np.uint32), 65)
    with pytest.raises(_lib.NmzInvalidArgument, match="strictly increasing"):
        hs.move_profile(ts, np.zeros((0, 2), np.uint32), 8, usym=[3, 3])


def test_script_moves_host_refusals_and_edges():
    L = _lib.load()
    a, b = np.array([1, 2, 3], np.uint64), np.array([2, 3, 1, 4], np.uint64)
    ops = np.zeros(2, _lib.EDIT_OP_DTYPE)
    ops[0], ops[1] = (0, 0, AR.DEL), (3, 2, AR.INS)
    pr = np.zeros(2, np.uint32)

    def call(pa=a, n=3, pb=b, m=4, o=ops, k=2, out=pr):
        return L.nmz_script_moves_host(_lib.ptr(pa), n, _lib.ptr(pb), m, _lib.ptr(o), k, _lib.ptr(out))

    assert call() == _lib.NMZ_OK and pr.tolist() == [1, 0]
    assert call(k=0, o=None, out=None) == _lib.NMZ_OK
    for kw, msg in [({"pa": None}, "a or b is NULL"), ({"pb": None}, "a or b is NULL"), ({"o": None}, "ops or partner is NULL"),
                    ({"out": None}, "ops or partner is NULL"), ({"n": 0}, "a_pos 0 is outside a trace of 0 elements (slot 0)"),
                    ({"m": 2}, "b_pos 2 is outside a trace of 2 elements (slot 1)")]:
        assert call(**kw) == _lib.NMZ_EINVAL and msg in _lib.last_error(), (kw, _lib.last_error())
    bad = ops.copy()
    bad[1]["kind"] = NONE  # a sentinel is no op
    assert call(o=bad) == _lib.NMZ_EINVAL and "op kind 4294967295 is not SUB, DEL or INS (slot 1)" in _lib.last_error()
    # a repeated symbol: the r-th DEL pairs with the r-th INS; the DEL left over has no partner
    a2, b2 = np.array([ord(c) for c in "xxabc"], np.uint64), np.array([ord(c) for c in "abcx"], np.uint64)
    d, sc = hs.edit_script_host(a2, b2, 4)
    assert d == 3 and hs.script_partners(a2, b2, sc).tolist() == [2, NONE, 0]


def test_top_ranks_by_scripts_then_moves_then_symbol():
    counts = np.zeros(5, _lib.MOVE_COUNTS_DTYPE)
    counts["n_pairs"] = [3, 5, 3, 0, 3]
    counts["later"] = [1, 0, 2, 0, 1]
    counts["earlier"] = [1, 0, 0, 0, 1]
    prof = hs.MoveProfile(np.array([10, 20, 30, 40, 50], np.uint64), counts, None, None)
    assert [s for s, _ in prof.top(10)] == [20, 10, 30, 50] and [s for s, _ in prof.top(2)] == [20, 10]
