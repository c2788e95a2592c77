"""CPU: the wide edit script's host form (nmz_ed_align_wide_host, bands up to 1,024) against the definition.

tests/align_ref.py is the definition in pure Python. The host form is tied to it op for op at bands beyond 64, to
the narrow host form (nmz_ed_align_host at band 64) on pairs within 64 edits, to answers known by construction at
the wide sizes, and to tests/golden/edit_script_kat.json. tests/test_align_wide_gpu.py takes its expected values
from this host form. Every comparison is integer equality, slot for slot."""
import ctypes
import functools

import numpy as np
import pytest

import align_ref as AR
import ed_cases as EC
from namazu_amd import _lib
from namazu_amd import historystorage as hs

NONE3 = (_lib.NMZ_NONE,) * 3
S, D, I = AR.SUB, AR.DEL, AR.INS


def wide_slots(a, b, w):
    """(dist, ops[w]) of nmz_ed_align_wide_host: all `band` slots, sentinels included."""
    a, b = np.ascontiguousarray(a, np.uint64), np.ascontiguousarray(b, np.uint64)
    dist = ctypes.c_uint32()
    ops = np.zeros(w, _lib.EDIT_OP_DTYPE)
    _lib.check(_lib.load().nmz_ed_align_wide_host(_lib.ptr(a), len(a), _lib.ptr(b), len(b), w, ctypes.byref(dist),
                                                  _lib.ptr(ops) if w else None))
    return dist.value, ops


def wide(a, b, w):
    d, sc = hs.edit_script_wide_host(a, b, w)
    return d, (None if sc is None else AR.as_tuples(sc))


# ---- 1. the definition, beyond 64 ------------------------------------------------------------------------------------
def _run_edits(a, n_del, n_ins, n_sub, rng):
    """a with n_del elements deleted and n_ins inserted, each in a few runs, and n_sub substituted."""
    t = list(a)
    for total, ins in ((n_del, False), (n_ins, True)):
        left = total
        while left:
            k = min(left, int(rng.integers(1, 24)))
            p = int(rng.integers(0, len(t) - (0 if ins else k) + 1))
            t[p:p + (0 if ins else k)] = [int(x) for x in rng.integers(0, 4, size=k)] if ins else []
            left -= k
    for _ in range(n_sub):
        p = int(rng.integers(0, len(t)))
        t[p] = (t[p] + 1 + int(rng.integers(0, 3))) % 4
    return t


@functools.lru_cache(maxsize=None)
def definition_pairs(w):
    """24 pairs over {0, 1, 2, 3}, lengths <= 200: 12 aimed between 65 and w edits (runs of deletes and inserts,
    so the path leaves the diagonal), 7 aimed beyond w at lengths within w of each other, so that the cut-off decides
    (over disjoint halves of the alphabet, where Lev = the longer length, or a trace of mostly one symbol that the
    other lacks), 5 near. Where each pair lands is the reference's to say."""
    rng = np.random.default_rng(1000 + w)
    out = []
    for t in range(12):
        a = [int(x) for x in rng.integers(0, 4, size=200)]
        # e edits, x of them not deletes: Lev >= the length difference >= e - 2 x >= 65, and Lev <= e <= w
        x = t % 3 if w >= 70 else 0
        e = int(rng.integers(65 + 2 * x, w + 1))
        b = _run_edits(a, e - x, x if t % 3 == 1 else 0, x if t % 3 == 2 else 0, rng)
        out.append((a, b) if t % 2 else (b, a))
    for t in range(7):
        n, m = int(rng.integers(150, 201)), int(rng.integers(150, 201))
        if t % 2:
            out.append(([int(x) for x in rng.integers(0, 2, size=n)], [int(x) for x in rng.integers(2, 4, size=m)]))
        else:  # b is 3s but for one place in seven, a has no 3: Lev >= n - m / 7 or so
            b = [int(x) if u < 1 else 3 for x, u in zip(rng.integers(0, 3, size=m), rng.integers(0, 7, size=m))]
            out.append(([int(x) for x in rng.integers(0, 3, size=n)], b))
    for t in range(5):
        a = [int(x) for x in rng.integers(0, 4, size=int(rng.integers(1, 200)))]
        out.append((a, _run_edits(a, min(t, len(a) - 1), 2 * t, t, rng)))
    return tuple(out)


@pytest.mark.parametrize("w", [65, 100, 130])
def test_wide_host_equals_definition(w):
    pairs = definition_pairs(w)
    lev = []
    for a, b in pairs:
        assert len(a) <= 200 and len(b) <= 200
        ref = AR.script(a, b, w)
        assert AR.script(a, b, w, band=w) == ref
        assert wide(a, b, w) == ref, (w, len(lev))
        lev.append(AR.matrix(a, b)[len(a)][len(b)] if ref[0] > w else ref[0])
    lev = np.array(lev)
    print(w, sorted(lev.tolist()))
    assert ((lev > 64) & (lev <= w)).sum() * 3 >= len(pairs)  # a third between 64 and the band
    assert (lev > w).sum() * 5 >= len(pairs)                  # a fifth beyond it


# ---- 2. band independence ------------------------------------------------------------------------------------------
def test_band_independence():
    """Within 64 edits the script at any wide band is the narrow form's at band 64, then sentinels."""
    trs = EC.traces("bv-w64")
    L = _lib.load()
    rng = np.random.default_rng(65)
    seen = 0
    for i, j in rng.integers(0, len(trs), size=(120, 2)).tolist():
        a, b = trs[i], trs[j]
        d64, o64 = ctypes.c_uint32(), np.zeros(64, _lib.EDIT_OP_DTYPE)
        _lib.check(L.nmz_ed_align_host(_lib.ptr(a), len(a), _lib.ptr(b), len(b), 64, ctypes.byref(d64), _lib.ptr(o64)))
        if d64.value > 64 or seen >= 30:
            continue
        seen += 1
        for w in (65, 1024):
            d, ops = wide_slots(a, b, w)
            assert d == d64.value and np.array_equal(ops[:64], o64), (i, j, w)
            assert AR.as_tuples(ops[64:]) == [NONE3] * (w - 64)
    assert seen == 30


@pytest.mark.parametrize("w", [0, 1, 8, 33, 64])
def test_narrow_bands_through_the_wide_host_form(w):
    trs = EC.traces("bv-w8")[:12]
    L = _lib.load()
    for a in trs:
        for b in trs:
            dn, on = ctypes.c_uint32(), np.zeros(w, _lib.EDIT_OP_DTYPE)
            _lib.check(L.nmz_ed_align_host(_lib.ptr(a), len(a), _lib.ptr(b), len(b), w, ctypes.byref(dn),
                                           _lib.ptr(on) if w else None))
            d, ops = wide_slots(a, b, w)
            assert d == dn.value and np.array_equal(ops, on)


# ---- 3. known answers by construction ----------------------------------------------------------------------------------
def constructed(w):
    """[(a, b, band, dist, script | None)] at the wide size w (int64 symbol ids): the table of the wide form's
    known answers. X = 1, Y = 2, B = a block of distinct symbols from 10 on. The rotation rows need an even band,
    so they use k = ceil(w / 2): bands 2 k and 2 k - 1."""
    X, Y = 1, 2

    def B(n):
        return list(range(10, 10 + n))

    k = (w + 1) // 2
    return [
        ([X] * w + B(7), B(7), w, w, [(t, 0, D) for t in range(w)]),
        (B(7), [X] * w + B(7), w, w, [(0, t, I) for t in range(w)]),
        ([X] * (w + 1) + B(2 * w + 5), B(2 * w + 5) + [Y] * (w + 1), w, w + 1, None),
        ([X] * k + B(3 * k), B(3 * k) + [X] * k, 2 * k, 2 * k,
         [(t, 0, D) for t in range(k)] + [(4 * k, 3 * k + t, I) for t in range(k)]),
        ([X] * k + B(3 * k), B(3 * k) + [X] * k, 2 * k - 1, 2 * k, None),
    ]


def test_constructed_answers_hold_in_the_definition():
    """The table at k = 5 (w = 10) against align_ref, full and banded matrix, and the wide host form there."""
    for a, b, band, dist, sc in constructed(10):
        assert AR.script(a, b, band) == (dist, sc) == AR.script(a, b, band, band=band)
        assert wide(EC.encode(a), EC.encode(b), band) == (dist, sc)


@pytest.mark.parametrize("w", [65, 1024])
def test_constructed_answers(w):
    for a, b, band, dist, sc in constructed(w):
        d, ops = wide_slots(EC.encode(a), EC.encode(b), band)
        assert d == dist
        want = (sc or []) + [NONE3] * (band - len(sc or []))
        assert AR.as_tuples(ops) == want, (w, band, dist)
        if sc is not None:
            assert len(sc) == dist and AR.replay(a, b, sc)


def test_known_answers_at_band_65(golden):
    rows = [c for c in golden("edit_script_kat.json") if c["script"] is not None]
    assert len(rows) >= 10
    for c in rows:
        a = np.array([ord(ch) for ch in c["a"]], np.uint64)
        b = np.array([ord(ch) for ch in c["b"]], np.uint64)
        assert wide(a, b, 65) == (c["dist"], [tuple(o) for o in c["script"]]), c


# ---- 4. limits: each refusal with its message and no device -------------------------------------------------------------
def test_wide_host_refusals():
    L = _lib.load()
    a, b = np.arange(3, dtype=np.uint64), np.arange(1, 4, dtype=np.uint64)
    dist = ctypes.c_uint32()
    ops = np.zeros(1025, _lib.EDIT_OP_DTYPE)
    for args, msg in [
        ((_lib.ptr(a), 3, _lib.ptr(b), 3, 1025, ctypes.byref(dist), _lib.ptr(ops)),
         "band 1025 exceeds NMZ_ALIGN_WIDE_MAX_BAND (1024)"),
        ((_lib.ptr(a), 2**32 - 1, _lib.ptr(b), 3, 70, ctypes.byref(dist), _lib.ptr(ops)), "a has 4294967295 elements"),
        ((_lib.ptr(a), 3, _lib.ptr(b), 2**32 - 1, 70, ctypes.byref(dist), _lib.ptr(ops)), "b has 4294967295 elements"),
        ((None, 3, _lib.ptr(b), 3, 70, ctypes.byref(dist), _lib.ptr(ops)), "a or b is NULL"),
        ((_lib.ptr(a), 3, None, 3, 70, ctypes.byref(dist), _lib.ptr(ops)), "a or b is NULL"),
        ((_lib.ptr(a), 3, _lib.ptr(b), 3, 70, None, _lib.ptr(ops)), "dist is NULL"),
        ((_lib.ptr(a), 3, _lib.ptr(b), 3, 70, ctypes.byref(dist), None), "ops is NULL"),
    ]:
        assert L.nmz_ed_align_wide_host(*args) == _lib.NMZ_EINVAL
        assert msg in _lib.last_error(), _lib.last_error()
    with pytest.raises(_lib.NmzInvalidArgument, match="wider bands are not built yet"):
        hs.edit_script_wide_host(a, b, 1025)
    assert L.nmz_ed_align_wide_host(None, 0, None, 0, 0, ctypes.byref(dist), None) == _lib.NMZ_OK and dist.value == 0
    assert _lib.NMZ_ALIGN_WIDE_MAX_BAND == 1024 and _lib.NMZ_ALIGN_MAX_BAND == 64


def test_wide_pairs_refusals_need_no_device():
    """Every limit of nmz_ed_align_wide_pairs and of the plan is checked before the context (ctx = NULL)."""
    L = _lib.load()
    sym = np.arange(8, dtype=np.uint64)
    off = np.array([0, 3, 3, 8], np.uint64)
    pairs = np.array([[0, 2], [1, 1]], np.uint32)
    dist = np.zeros(2, np.uint32)
    ops = np.zeros((2, 1024), _lib.EDIT_OP_DTYPE)

    def call(off=off, sym=sym, n_traces=3, pairs=pairs, n_pairs=2, band=100, dist=dist, ops=ops):
        return L.nmz_ed_align_wide_pairs(None, _lib.ptr(off), _lib.ptr(sym), n_traces, _lib.ptr(pairs), n_pairs, band,
                                         _lib.ptr(dist), _lib.ptr(ops))

    for kw, msg in [
        ({}, "ctx is NULL"),
        ({"band": 8}, "ctx is NULL"),
        ({"band": 1024}, "ctx is NULL"),
        ({"band": 1025}, "band 1025 exceeds NMZ_ALIGN_WIDE_MAX_BAND (1024)"),
        ({"band": 1025}, "wider bands are not built yet"),
        ({"pairs": np.array([[0, 3], [1, 1]], np.uint32)}, "pair index out of range (pair 0)"),
        ({"off": np.array([0, 5, 3, 8], np.uint64)}, "offsets must be non-decreasing (trace 1)"),
        ({"off": np.array([0, 2**32 - 1, 2**32, 2**32], np.uint64)}, "trace 0 has 4294967295 elements"),
        ({"off": None}, "off, pairs or dist is NULL"),
        ({"pairs": None}, "off, pairs or dist is NULL"),
        ({"dist": None}, "off, pairs or dist is NULL"),
        ({"ops": None}, "ops is NULL"),
        ({"sym": None}, "sym is NULL"),
    ]:
        assert call(**kw) == _lib.NMZ_EINVAL, kw
        assert msg in _lib.last_error(), (kw, _lib.last_error())
    assert call(n_pairs=0) == _lib.NMZ_OK  # legal, and needs no device
    assert call(n_pairs=0, band=1024, ops=None, dist=None) == _lib.NMZ_OK
    assert call(n_pairs=0, band=1025) == _lib.NMZ_EINVAL
    assert "NMZ_ALIGN_WIDE_MAX_BAND (1024)" in _lib.last_error()
    es = hs.edit_scripts_wide(hs.TraceSet([sym[:3], sym[3:]]), np.zeros((0, 2), np.uint32), 300)
    assert es.dist.shape == (0,) and es.ops.shape == (0, 300)
    with pytest.raises(_lib.NmzInvalidArgument, match="wider bands are not built yet"):
        hs.edit_scripts_wide(hs.TraceSet([sym[:3], sym[3:]]), np.array([[0, 1]], np.uint32), 1025)
    # the plan and the device form
    plan = ctypes.c_void_p(1)
    for band in (8, 65, 1024):
        assert L.nmz_ed_align_wide_plan_create(None, band, 100, ctypes.byref(plan)) == _lib.NMZ_EINVAL
        assert not plan.value and "ctx is NULL" in _lib.last_error()
    assert L.nmz_ed_align_wide_plan_create(None, 1025, 100, ctypes.byref(plan)) == _lib.NMZ_EINVAL
    assert "band 1025 exceeds NMZ_ALIGN_WIDE_MAX_BAND (1024)" in _lib.last_error()
    assert L.nmz_ed_align_wide_plan_create(None, 1024, 2**20, ctypes.byref(plan)) == _lib.NMZ_EINVAL
    assert "max_len 1048576" in _lib.last_error() and "budget of 268435456 bytes" in _lib.last_error()
    assert L.nmz_ed_align_wide_plan_create(None, 1024, 400000, ctypes.byref(plan)) == _lib.NMZ_EINVAL
    assert "ctx is NULL" in _lib.last_error()  # 400,000 rows of 576 bytes fit the budget
    assert L.nmz_ed_align_wide_plan_create(None, 100, 2**32 - 1, ctypes.byref(plan)) == _lib.NMZ_EINVAL
    assert L.nmz_ed_align_wide_plan_create(None, 100, 100, None) == _lib.NMZ_EINVAL
    assert L.nmz_ed_align_wide_plan_destroy(None) == _lib.NMZ_OK
    assert L.nmz_ed_align_wide_plan_info(None, None, None) == _lib.NMZ_EINVAL
    assert L.nmz_ed_align_wide_pairs_dev(None, None, None, None, 1, None, None, None) == _lib.NMZ_EINVAL
    assert "plan is NULL" in _lib.last_error()
