"""CPU: the edit script's host form (nmz_ed_align_host) against the definition.

tests/align_ref.py is the definition in pure Python; tests/golden/edit_script_kat.json holds known answers made by
a third, independent program. The host form is tied to both here, op for op, on the structured families of
tests/ed_cases.py -- and the counts below show that those families exercise the tie rule, all three op kinds, the
band's edge and a script as long as the band, so the GPU comparison (tests/test_align_gpu.py, which takes its
expected values from the host form) cannot pass vacuously."""
import ctypes
import functools

import numpy as np
import pytest

import align_ref as AR
import ed_cases as EC
from namazu_amd import _lib
from namazu_amd import historystorage as hs

BV = ["bv-w5", "bv-w8", "bv-w16", "bv-w32", "bv-w33", "bv-w50", "bv-w64", "bv-per8", "bv-per32", "bv-per64"]
FULL = ["bv-w5", "bv-w8", "bv-w16", "bv-per8"]  # the definition on the unrestricted matrix
PERIODIC = [n for n in BV if "per" in n]
NONE3 = (_lib.NMZ_NONE,) * 3


def enc(s):
    return np.array([ord(c) for c in s], np.uint64)


@functools.lru_cache(maxsize=None)
def ref_scripts(name):
    """{(i, j): (ops, cells, ops under the reversed preference)} for the in-band ordered pairs of a case, from
    align_ref (and the oracle's distances to pick the pairs): the full matrix for FULL, else the banded one."""
    trs, D, w = EC.traces(name), EC.reference(name), EC.band(name)
    out = {}
    for i in range(len(trs)):
        for j in range(len(trs)):
            if D[i, j] > w:
                continue
            a, b = trs[i].tolist(), trs[j].tolist()
            M = AR.matrix(a, b, None if name in FULL else w)
            assert M[len(a)][len(b)] == D[i, j]
            ops, cells = AR.walk(a, b, M)
            alt, _ = AR.walk(a, b, M, prefer=("left", "up", "diag"))
            out[(i, j)] = (ops, cells, alt)
    return out


def host(a, b, w):
    d, sc = hs.edit_script_host(a, b, w)
    return d, (None if sc is None else AR.as_tuples(sc))


# ---- 1. the fixture -----------------------------------------------------------------------------------------------
def test_known_answers(golden):
    kat = golden("edit_script_kat.json")
    assert len(kat) >= 20
    for c in kat:
        a, b, w = enc(c["a"]), enc(c["b"]), c["band"]
        want = None if c["script"] is None else [tuple(o) for o in c["script"]]
        assert AR.script(a, b, w) == (c["dist"], want), c
        assert host(a, b, w) == (c["dist"], want), c
        if want is not None:
            assert AR.replay(a, b, want) and len(want) == c["dist"]
    # the table of DESIGN.md section 2, spelled out
    S, D, I = AR.SUB, AR.DEL, AR.INS
    table = {("kitten", "sitting", 3): (3, [(0, 0, S), (4, 4, S), (6, 6, I)]), ("kitten", "sitting", 2): (3, None),
             ("abc", "", 3): (3, [(0, 0, D), (1, 0, D), (2, 0, D)]), ("", "ab", 2): (2, [(0, 0, I), (0, 1, I)]),
             ("ab", "ba", 2): (2, [(0, 0, S), (1, 1, S)]), ("aab", "ab", 1): (1, [(0, 0, D)]),
             ("ab", "aab", 1): (1, [(0, 0, I)]), ("abcde", "bcdex", 2): (2, [(0, 0, D), (5, 4, I)]),
             ("abab", "baba", 2): (2, [(0, 0, I), (3, 4, D)]), ("aaaa", "aa", 2): (2, [(0, 0, D), (1, 0, D)])}
    by_key = {(c["a"], c["b"], c["band"]): c for c in kat}
    for key, (dist, want) in table.items():
        c = by_key[key]
        assert c["dist"] == dist and (c["script"] if want is None else [tuple(o) for o in c["script"]]) == want


# ---- 2. the host form, op for op ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FULL)
def test_host_equals_definition(name):
    trs, D, w = EC.traces(name), EC.reference(name), EC.band(name)
    ref = ref_scripts(name)
    for i in range(len(trs)):
        for j in range(len(trs)):
            d, sc = host(trs[i], trs[j], w)
            assert d == D[i, j]
            assert sc == (ref[(i, j)][0] if (i, j) in ref else None), (name, i, j)


def test_host_equals_definition_w64_sample():
    """40 in-band pairs of bv-w64 (every third cell of the band per lane, the extra cell of w = 64) on the full
    matrix."""
    trs, D, w = EC.traces("bv-w64"), EC.reference("bv-w64"), 64
    inb = [(i, j) for i in range(len(trs)) for j in range(len(trs)) if i != j and D[i, j] <= w]
    rng = np.random.default_rng(64)
    for i, j in [inb[t] for t in rng.choice(len(inb), 40, replace=False)]:
        assert host(trs[i], trs[j], w) == AR.script(trs[i].tolist(), trs[j].tolist(), w), (i, j)


def test_full_and_banded_matrix_agree():
    """The definition's matrix and the +inf-banded one give the same script wherever Lev <= w (bv-w8)."""
    trs, w = EC.traces("bv-w8"), 8
    for (i, j), (ops, _, _) in ref_scripts("bv-w8").items():
        assert AR.script(trs[i].tolist(), trs[j].tolist(), w, band=w) == (len(ops), ops)


@pytest.mark.parametrize("name", BV)
def test_host_scripts_replay(name):
    trs, D, w = EC.traces(name), EC.reference(name), EC.band(name)
    ref = ref_scripts(name)
    for i in range(len(trs)):
        for j in range(len(trs)):
            d, sc = host(trs[i], trs[j], w)
            assert d == D[i, j]
            if d > w:
                assert sc is None
                continue
            assert len(sc) == d and AR.replay(trs[i], trs[j], sc), (name, i, j)
            assert sc == ref[(i, j)][0], (name, i, j)  # banded reference beyond FULL
            if d == 0:
                assert np.array_equal(trs[i], trs[j])  # an empty script <=> Equals


# ---- 3. non-vacuity, from align_ref and the oracle alone ------------------------------------------------------------
@pytest.mark.parametrize("name", BV)
def test_families_exercise_the_rule(name):
    w, ref = EC.band(name), ref_scripts(name)
    off = {k: v for k, v in ref.items() if k[0] != k[1]}
    in_band = len(off)
    tie = sum(ops != alt for ops, _, alt in off.values())
    kinds3 = sum(len({k for _, _, k in ops}) == 3 for ops, _, _ in off.values())
    edge = sum(any(abs(i - j) == w for i, j in cells) for _, cells, _ in off.values())
    longest = max(len(ops) for ops, _, _ in off.values())
    print(name, dict(in_band=in_band, tie=tie, kinds3=kinds3, edge=edge, longest=longest))
    if name in PERIODIC:
        assert tie >= 8 and edge >= 2
    else:
        assert in_band >= 300 and tie >= 140 and kinds3 >= 30 and edge >= 30
        assert longest == w


# ---- 4. refusals and edges ------------------------------------------------------------------------------------------
def test_host_refusals():
    L = _lib.load()
    a, b = enc("abc"), enc("abd")
    dist = ctypes.c_uint32()
    ops = np.zeros(65, _lib.EDIT_OP_DTYPE)

    def call(pa, n, pb, m, band, pd, po):
        return L.nmz_ed_align_host(pa, n, pb, m, band, pd, po)

    for args, msg in [
        ((_lib.ptr(a), 3, _lib.ptr(b), 3, 65, ctypes.byref(dist), _lib.ptr(ops)), "exceeds NMZ_ALIGN_MAX_BAND (64)"),
        ((_lib.ptr(a), 2**32 - 1, _lib.ptr(b), 3, 4, ctypes.byref(dist), _lib.ptr(ops)), "a has 4294967295 elements"),
        ((_lib.ptr(a), 3, _lib.ptr(b), 2**32 - 1, 4, ctypes.byref(dist), _lib.ptr(ops)), "b has 4294967295 elements"),
        ((None, 3, _lib.ptr(b), 3, 4, ctypes.byref(dist), _lib.ptr(ops)), "a or b is NULL"),
        ((_lib.ptr(a), 3, None, 3, 4, ctypes.byref(dist), _lib.ptr(ops)), "a or b is NULL"),
        ((_lib.ptr(a), 3, _lib.ptr(b), 3, 4, None, _lib.ptr(ops)), "dist is NULL"),
        ((_lib.ptr(a), 3, _lib.ptr(b), 3, 4, ctypes.byref(dist), None), "ops is NULL"),
    ]:
        assert call(*args) == _lib.NMZ_EINVAL
        assert msg in _lib.last_error()
    with pytest.raises(_lib.NmzInvalidArgument, match="wider bands are not built yet"):
        hs.edit_script_host(a, b, 65)


def test_pairs_refusals_need_no_device():
    """Every limit of nmz_ed_align_pairs is checked before the context: a NULL context never gets that far."""
    L = _lib.load()
    sym = np.arange(8, dtype=np.uint64)
    off = np.array([0, 3, 3, 8], np.uint64)
    pairs = np.array([[0, 2], [1, 1]], np.uint32)
    dist = np.zeros(2, np.uint32)
    ops = np.zeros((2, 64), _lib.EDIT_OP_DTYPE)

    def call(off=off, n_traces=3, pairs=pairs, n_pairs=2, band=8, dist=dist, ops=ops):
        return L.nmz_ed_align_pairs(None, _lib.ptr(off), _lib.ptr(sym), n_traces, _lib.ptr(pairs), n_pairs, band,
                                    _lib.ptr(dist), _lib.ptr(ops))

    for kw, msg in [
        ({}, "ctx is NULL"),
        ({"band": 65}, "wider bands are not built yet"),
        ({"pairs": np.array([[0, 3], [1, 1]], np.uint32)}, "pair index out of range (pair 0)"),
        ({"off": np.array([0, 5, 3, 8], np.uint64)}, "offsets must be non-decreasing (trace 1)"),
        ({"off": np.array([0, 2**32 - 1, 2**32, 2**32], np.uint64)}, "trace 0 has 4294967295 elements"),
        ({"dist": None}, "off, pairs or dist is NULL"),
        ({"ops": None}, "ops is NULL"),
    ]:
        assert call(**kw) == _lib.NMZ_EINVAL, kw
        assert msg in _lib.last_error(), (kw, _lib.last_error())
    assert call(n_pairs=0) == _lib.NMZ_OK  # legal, and needs no device
    assert call(n_pairs=0, band=65) == _lib.NMZ_EINVAL
    es = hs.edit_scripts(hs.TraceSet([sym[:3], sym[3:]]), np.zeros((0, 2), np.uint32), 8)
    assert es.dist.shape == (0,) and es.ops.shape == (0, 8)
    # the plan and the device form
    plan = ctypes.c_void_p(1)
    assert L.nmz_ed_align_plan_create(None, 8, 100, ctypes.byref(plan)) == _lib.NMZ_EINVAL and not plan.value
    assert "ctx is NULL" in _lib.last_error()
    assert L.nmz_ed_align_plan_create(None, 65, 100, ctypes.byref(plan)) == _lib.NMZ_EINVAL
    assert "NMZ_ALIGN_MAX_BAND" in _lib.last_error()
    assert L.nmz_ed_align_plan_create(None, 64, 2**30, ctypes.byref(plan)) == _lib.NMZ_EINVAL
    assert "max_len 1073741824" in _lib.last_error() and "budget" in _lib.last_error()
    assert L.nmz_ed_align_plan_create(None, 8, 2**32 - 1, ctypes.byref(plan)) == _lib.NMZ_EINVAL
    assert L.nmz_ed_align_plan_destroy(None) == _lib.NMZ_OK
    assert L.nmz_ed_align_plan_info(None, None, None) == _lib.NMZ_EINVAL
    assert L.nmz_ed_align_pairs_dev(None, None, None, None, 1, None, None, None) == _lib.NMZ_EINVAL
    assert "plan is NULL" in _lib.last_error()


def test_host_edges():
    e = np.zeros(0, np.uint64)
    assert host(e, e, 0) == (0, []) and host(e, e, 5) == (0, [])
    assert host(enc("abc"), enc("abc"), 0) == (0, [])
    assert host(enc("abc"), enc("abd"), 0) == (1, None) and host(enc("abc"), enc("ab"), 0) == (1, None)
    assert host(e, enc("ab"), 2) == (2, [(0, 0, AR.INS), (0, 1, AR.INS)])
    assert host(enc("ab"), e, 2) == (2, [(0, 0, AR.DEL), (1, 0, AR.DEL)])
    assert host(e, enc("abc"), 2) == (3, None)
    # dist == w exactly, and w + 1: substitutions spread over a trace
    for w in (1, 7, 64):
        a = np.arange(300, dtype=np.uint64)
        for k, in_band in ((w, True), (w + 1, False)):
            b = a.copy()
            at = np.arange(k) * 4 + 1
            b[at] += np.uint64(1000)
            d, sc = host(a, b, w)
            assert d == k
            assert sc == ([(int(p), int(p), AR.SUB) for p in at] if in_band else None)
    # the sentinel behind a script, and a full one
    L = _lib.load()
    ops = np.zeros(4, _lib.EDIT_OP_DTYPE)
    dist = ctypes.c_uint32()
    a, b = enc("kitten"), enc("sitting")
    assert L.nmz_ed_align_host(_lib.ptr(a), 6, _lib.ptr(b), 7, 4, ctypes.byref(dist), _lib.ptr(ops)) == 0
    assert dist.value == 3 and AR.as_tuples(ops) == [(0, 0, AR.SUB), (4, 4, AR.SUB), (6, 6, AR.INS), NONE3]
    assert L.nmz_ed_align_host(_lib.ptr(a), 6, _lib.ptr(b), 7, 2, ctypes.byref(dist), _lib.ptr(ops)) == 0
    assert dist.value == 3 and AR.as_tuples(ops[:2]) == [NONE3, NONE3]


# ---- 5. script_moves -----------------------------------------------------------------------------------------------
def test_script_moves():
    a = EC.encode(np.arange(40))
    rot = np.concatenate([a[3:], a[:3]])
    d, sc = hs.edit_script_host(a, rot, 8)
    assert d == 6
    assert hs.script_moves(a, rot, sc) == [(int(a[k]), k, 37 + k) for k in range(3)]
    sub = a.copy()
    sub[17] = np.uint64(99)
    d, sc = hs.edit_script_host(a, sub, 8)
    assert d == 1 and hs.script_moves(a, sub, sc) == []
    # a repeated symbol: the k-th DEL pairs with the k-th INS of that value; an unpaired DEL is no move
    a2, b2 = enc("xxabc"), enc("abcx")
    d, sc = hs.edit_script_host(a2, b2, 4)
    assert d == 3 and hs.script_moves(a2, b2, sc) == [(ord("x"), 0, 3)]
