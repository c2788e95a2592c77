"""CPU: the wide move profile's host form (nmz_move_profile_wide_host) against the definition.

tests/moves_ref.py is the definition in pure Python; tests/moves_wide_cases.py holds constructed rows whose profile
has a closed form at any size, and a moved-block family whose scripts run to 543 ops. The rows are tied to the plain
matrix (tests/align_ref.py) at k = 5 and to their closed forms at k = 33 (band 66: the first scripts past one wave)
and k = 512 (band 1,024). On the family the scripts are the wide host aligner's, which
tests/test_align_wide_host.py ties to the definition, so the restatement here covers pairing and tally. The counts
asserted below show that the GPU comparison (tests/test_moves_wide_gpu.py, which takes its expected values from this
host form) cannot pass vacuously."""
import ctypes
import functools

import numpy as np
import pytest

import align_ref as AR
import moves_cases as MC
import moves_ref as MR
import moves_wide_cases as WC
from namazu_amd import _lib
from namazu_amd import historystorage as hs
from test_moves_host import check_profile, table_of

NONE = _lib.NMZ_NONE


def row_profile(r):
    """(EditScripts, MoveProfile with partners) of one constructed row through the wide host forms."""
    trs = [MC.encode(r["a"]), MC.encode(r["b"])]
    es = WC.host_scripts_wide(trs, [(0, 1)], r["band"])
    usym, ids = table_of(set(r["a"]) | set(r["b"]))
    prof = hs.move_profile_of_wide(hs.TraceSet(trs), [[0, 1]], es, usym=usym, want_partner=True, host=True)
    return trs, es, ids, prof


def check_row(r, es, ids, prof):
    """One constructed row's EditScripts and MoveProfile (pair 0) against its closed forms."""
    d, w = r["dist"], r["band"]
    assert int(es.dist[0]) == int(prof.dist[0]) == d, r["name"]
    if r["kinds"] is None:
        assert d == w + 1 and (prof.partner[0] == NONE).all()
        return
    assert es.ops[0, :d]["kind"].tolist() == r["kinds"], r["name"]
    want = np.full(w, NONE, np.uint32)
    want[:d] = [NONE if q is None else q for q in r["partner"]]
    assert np.array_equal(prof.partner[0], want), (r["name"], np.nonzero(prof.partner[0] != want)[0][:8])
    for u, v in enumerate(ids):
        got = {f: int(prof.counts[u][f]) for f in MR.FIELDS}
        assert got == r["counts"].get(v, WC.ZERO), (r["name"], v, got)


# ---- 1. the constructed rows ---------------------------------------------------------------------------------------
def test_constructed_rows_equal_the_definition_at_k5():
    """The closed forms against the plain matrix and the pure-Python tally, then the host forms against both."""
    for r in WC.constructed(5, j=2):
        a, b, w = r["a"], r["b"], r["band"]
        dist, ops = AR.script(a, b, w, band=w)
        assert dist == r["dist"] and (ops is None) == (r["kinds"] is None), r["name"]
        partner, counts, info, _ = MR.profile([a, b], [(0, 1)], w)
        assert counts == r["counts"] and info == r["info"], r["name"]
        trs, es, ids, prof = row_profile(r)
        check_profile(prof, ids, counts, info, partner)
        check_row(r, es, ids, prof)
        if ops is not None:
            assert [op[2] for op in ops] == r["kinds"] and partner[0][:dist] == r["partner"]
            assert AR.as_tuples(es.script(0)) == ops


@pytest.mark.parametrize("k", [33, 512])
def test_constructed_rows_equal_their_closed_forms(k):
    rows = WC.constructed(k)
    for r in rows:
        trs, es, ids, prof = row_profile(r)
        check_row(r, es, ids, prof)
        assert {f: int(prof.info[f]) for f in r["info"]} == r["info"], r["name"]
        if r["kinds"] is not None:  # nmz_script_moves_host agrees on the partners
            got = hs.script_partners(trs[0], trs[1], es.script(0))
            assert [None if q == NONE else int(q) for q in got] == r["partner"], r["name"]
    if k == 512:
        rot = rows[0]["counts"][WC.X]
        assert rows[0]["band"] == 1024 and rot["later"] == 512 and rot["span_later"] == 917248
        assert rows[0]["partner"][511] == 1023 and rows[0]["partner"][1023] == 511


# ---- 2. the moved-block family -------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def family_ref(w):
    """(pairs, scripts {(i, j): (dist, ops | None)} of the wide host aligner, moves_ref.profile over them)."""
    fam = WC.family()
    trs = WC.family_encoded()
    pairs = MC.ordered_pairs(len(fam))
    scripts = {}
    for i, j in pairs:
        d, o = WC.wide_slots(trs[i], trs[j], w)
        scripts[(i, j)] = (d, AR.as_tuples(o[:d]) if d <= w else None)
    return pairs, scripts, MR.profile(fam, pairs, w, scripts=scripts)


# per band: scripts, beyond, dist in 65 .. band, dist in 257 .. band, later + earlier moves, partnered slots that are
# at least 256 apart (None: not asserted at that band)
FAMILY_AT = {256: (84, 98, 72, None, 4225, None), 512: (168, 14, 156, 84, 15004, 360),
             1024: (182, 0, 170, 98, None, 956)}


@pytest.mark.parametrize("w", sorted(FAMILY_AT))
def test_family_equals_definition(w):
    fam = WC.family()
    assert len(fam) == 14 and {x for t in fam for x in t} == set(range(40))
    pairs, scripts, (partner, counts, info, dist) = family_ref(w)
    assert len(pairs) == 182
    trs = WC.family_encoded()
    usym, ids = table_of(set(range(40)))
    es = WC.host_scripts_wide(trs, pairs, w)
    assert es.dist.tolist() == dist
    prof = hs.move_profile_of_wide(hs.TraceSet(list(trs)), pairs, es, usym=usym, want_partner=True, host=True)
    check_profile(prof, ids, counts, info, partner)
    plain = hs.move_profile_of_wide(hs.TraceSet(list(trs)), pairs, es, usym=usym, host=True)  # partner == NULL
    assert plain.partner is None and plain.counts.tobytes() == prof.counts.tobytes() and plain.info == prof.info
    # non-vacuity
    n_scripts, n_beyond, n_wide, n_257, n_moves, n_far = FAMILY_AT[w]
    d = np.array(dist)
    moves = int(prof.counts["later"].sum() + prof.counts["earlier"].sum())
    slot = np.arange(w, dtype=np.int64)[None, :]
    far = int(((prof.partner != NONE) & (np.abs(prof.partner.astype(np.int64) - slot) >= 256)).sum())
    print(w, dict(scripts=info["n_scripts"], beyond=info["n_beyond"], wide=int(((d > 64) & (d <= w)).sum()),
                  over256=int(((d > 256) & (d <= w)).sum()), moves=moves, far=far, max_dist=int(d[d <= w].max())))
    assert info["n_scripts"] >= n_scripts and info["n_beyond"] >= n_beyond and info["n_unknown"] == 0
    assert ((d > 64) & (d <= w)).sum() >= n_wide
    assert n_257 is None or ((d > 256) & (d <= w)).sum() >= n_257
    assert n_moves is None or moves >= n_moves
    assert n_far is None or far >= n_far


def test_family_exercises_the_rule():
    """At band 1,024: the longest script, a value that moves 13 times in one script, values with unequal DEL and INS
    counts and scripts with moves in both directions."""
    fam = WC.family()
    pairs, scripts, _ = family_ref(1024)
    both = unequal = most = 0
    for i, j in pairs:
        d, ops = scripts[(i, j)]
        if d <= 64:
            continue
        lt, el, _, un = MR.script_kinds(fam[i], fam[j], ops)
        both, unequal = both + (lt and el), unequal + un
        per_value = {}
        for v, *_ in MR.moves(fam[i], fam[j], ops):
            per_value[v] = per_value.get(v, 0) + 1
        most = max([most] + list(per_value.values()))
    assert max(d for d, _ in scripts.values()) == 543
    assert most >= 13 and unequal >= 110 and both >= 46


# ---- 3. bands <= 64 through the wide host form -----------------------------------------------------------------------
@pytest.mark.parametrize("w", [0, 8, 31, 64])
def test_narrow_bands_equal_the_narrow_host_form(w):
    fam = MC.family(31)
    trs = [MC.encode(t) for t in fam]
    pairs = MC.ordered_pairs(len(fam))
    ts = hs.TraceSet(trs)
    es = MC.host_scripts(trs, pairs, w)
    narrow = hs.move_profile_of(ts, pairs, es, want_partner=True, host=True)
    wide = hs.move_profile_of_wide(ts, pairs, es, want_partner=True, host=True)
    assert wide.counts.tobytes() == narrow.counts.tobytes() and wide.info.tobytes() == narrow.info.tobytes()
    assert wide.partner.tobytes() == narrow.partner.tobytes() and wide.partner.shape == (len(pairs), w)
    assert int(narrow.info["n_scripts"]) >= (100 if w else 30) and int(narrow.info["n_beyond"]) >= 100


# ---- 4. refusals and edges -------------------------------------------------------------------------------------------
def _small(band=8):
    sym = np.arange(8, dtype=np.uint64)
    off = np.array([0, 3, 3, 8], np.uint64)
    pairs = np.array([[0, 2], [1, 1]], np.uint32)
    dist = np.array([2, 0], np.uint32)
    ops = np.zeros((2, band), _lib.EDIT_OP_DTYPE)
    ops[:] = (NONE, NONE, NONE)
    ops[0, 0] = (0, 0, AR.DEL)
    ops[0, 1] = (3, 4, AR.INS)
    return sym, off, pairs, dist, ops


def test_wide_profile_refusals_need_no_device():
    """Every limit of the host-pointer forms is checked before the context: a NULL context never gets that far."""
    L = _lib.load()
    sym, off, pairs, dist, ops = _small()
    usym = np.arange(8, dtype=np.uint64)
    counts = np.zeros(8, _lib.MOVE_COUNTS_DTYPE)
    info = np.zeros(1, _lib.MOVE_INFO_DTYPE)
    partner = np.zeros((2, 1024), np.uint32)

    def forms(off=off, n_traces=3, pairs=pairs, n_pairs=2, band=8, dist=dist, ops=ops, usym=usym, n_usym=8,
              counts=counts, info=info, only=None):
        given = (_lib.ptr(off), _lib.ptr(sym), n_traces, _lib.ptr(pairs), n_pairs, band, _lib.ptr(dist), _lib.ptr(ops),
                 _lib.ptr(usym), n_usym, _lib.ptr(partner), _lib.ptr(counts), _lib.ptr(info))
        made = (None, _lib.ptr(off), _lib.ptr(sym), n_traces, _lib.ptr(pairs), n_pairs, band, _lib.ptr(usym), n_usym,
                _lib.ptr(dist), _lib.ptr(counts), _lib.ptr(info))
        out = {"host": lambda: L.nmz_move_profile_wide_host(*given),
               "given": lambda: L.nmz_move_profile_wide(None, *given),
               "made": lambda: L.nmz_ed_diff_profile_wide(*made)}
        return {k: f for k, f in out.items() if only is None or k in only}

    # a script of 301 ops at band 512 whose slot 300 is bad: the first 300 are DELs of a trace of 400 elements
    sym_l = np.arange(400, dtype=np.uint64)
    off_l = np.array([0, 400, 400], np.uint64)
    pairs_l = np.array([[0, 1]], np.uint32)
    dist_l = np.array([301], np.uint32)
    ops_l = np.zeros((1, 512), _lib.EDIT_OP_DTYPE)
    ops_l[:] = (NONE, NONE, NONE)
    for s in range(301):
        ops_l[0, s] = (s, 0, AR.DEL)

    alive = []

    def long_forms(op):
        o = ops_l.copy()
        o[0, 300] = op
        alive.append(o)  # the calls below hold its address only
        given = (_lib.ptr(off_l), _lib.ptr(sym_l), 2, _lib.ptr(pairs_l), 1, 512, _lib.ptr(dist_l), _lib.ptr(o),
                 _lib.ptr(usym), 8, _lib.ptr(partner), _lib.ptr(counts), _lib.ptr(info))
        return {"host": lambda: L.nmz_move_profile_wide_host(*given),
                "given": lambda: L.nmz_move_profile_wide(None, *given)}

    with_ops = ("host", "given")
    for kw, msg in [
        ({"band": 1025}, "NMZ_ALIGN_WIDE_MAX_BAND"),
        ({"band": 1024, "n_pairs": 2**22}, "n_pairs * band = 4194304 * 1024 must stay below 2^32"),
        ({"pairs": np.array([[0, 3], [1, 1]], np.uint32)}, "pair index out of range (pair 0)"),
        ({"off": np.array([0, 5, 3, 8], np.uint64)}, "offsets must be non-decreasing (trace 1)"),
        ({"off": np.array([0, 2**32 - 1, 2**32, 2**32], np.uint64)}, "trace 0 has 4294967295 elements"),
        ({"dist": None, "only": with_ops}, "off, pairs or dist is NULL"),
        ({"ops": None, "only": with_ops}, "ops is NULL"),
        ({"usym": None}, "usym or counts is NULL"),
        ({"counts": None}, "usym or counts is NULL"),
        ({"info": None}, "info is NULL"),
        ({"usym": np.array([0, 1, 2, 3, 3, 5, 6, 7], np.uint64)}, "usym must be strictly increasing (entry 4)"),
    ]:
        for name, f in forms(**kw).items():
            assert f() == _lib.NMZ_EINVAL, (name, kw)
            assert msg in _lib.last_error(), (name, kw, _lib.last_error())
    for op, msg in [((300, 0, 7), "op kind 7 is not SUB, DEL or INS (pair 0, slot 300)"),
                    ((400, 0, AR.DEL), "a_pos 400 is outside a trace of 400 elements (pair 0, slot 300)"),
                    ((300, 0, AR.INS), "b_pos 0 is outside a trace of 0 elements (pair 0, slot 300)")]:
        for name, f in long_forms(op).items():
            assert f() == _lib.NMZ_EINVAL and msg in _lib.last_error(), (name, op, _lib.last_error())
    assert long_forms((300, 0, AR.DEL))["host"]() == _lib.NMZ_OK and int(info[0]["n_ops"]) == 301
    # with valid arguments the device forms get as far as the context, at a narrow band and at a wide one
    for name in ("given", "made"):
        assert forms()[name]() == _lib.NMZ_EINVAL and "ctx is NULL" in _lib.last_error()
    assert long_forms((300, 0, AR.DEL))["given"]() == _lib.NMZ_EINVAL and "ctx is NULL" in _lib.last_error()
    for band in (8, 512, 1025):
        assert L.nmz_move_profile_wide_dev(None, None, None, None, 0, band, None, None, None, 0, None, None, None, 0,
                                           None) == _lib.NMZ_EINVAL and "ctx is NULL" in _lib.last_error()


def test_no_pairs_need_no_device():
    L = _lib.load()
    band = 512
    sym, off, pairs, dist, ops = _small(band)
    usym = np.arange(8, dtype=np.uint64)
    for form in ("host", "given", "made"):
        counts = np.full(8 * 12, 7, np.uint32).view(_lib.MOVE_COUNTS_DTYPE)
        info = np.full(8, 7, np.uint32).view(_lib.MOVE_INFO_DTYPE)
        if form == "made":
            rc = L.nmz_ed_diff_profile_wide(None, _lib.ptr(off), _lib.ptr(sym), 3, _lib.ptr(pairs), 0, band,
                                            _lib.ptr(usym), 8, None, _lib.ptr(counts), _lib.ptr(info))
        else:
            f = L.nmz_move_profile_wide_host if form == "host" else (lambda *a: L.nmz_move_profile_wide(None, *a))
            rc = f(_lib.ptr(off), _lib.ptr(sym), 3, _lib.ptr(pairs), 0, band, _lib.ptr(dist), _lib.ptr(ops),
                   _lib.ptr(usym), 8, None, _lib.ptr(counts), _lib.ptr(info))
        assert rc == _lib.NMZ_OK, (form, _lib.last_error())
        assert not counts.view(np.uint32).any() and not info.view(np.uint32).any()
    ts = hs.TraceSet([sym[:3], sym[3:]])
    empty = np.zeros((0, 2), np.uint32)
    made = dict(_lib._default_ctx)
    prof = hs.move_profile_wide(ts, empty, 8)  # no context is made for it
    assert _lib._default_ctx == made
    assert prof.symbols.tolist() == list(range(8)) and not prof.counts.view(np.uint32).any() and prof.top(3) == []
    assert prof.dist.shape == (0,) and int(prof.info["n_scripts"]) == 0
    wide = hs.move_profile_wide(ts, empty, 1024)
    assert int(wide.info["n_beyond"]) == 0 and not wide.counts.view(np.uint32).any()
    with pytest.raises(_lib.NmzInvalidArgument, match="NMZ_ALIGN_WIDE_MAX_BAND"):
        hs.move_profile_wide(ts, empty, 1025)
    with pytest.raises(_lib.NmzInvalidArgument, match="wider bands are not built yet"):
        hs.move_profile(ts, empty, 65)  # the narrow form keeps its limit
    with pytest.raises(_lib.NmzInvalidArgument, match="strictly increasing"):
        hs.move_profile_wide(ts, empty, 512, usym=[3, 3])
    es = hs.EditScripts(np.zeros(0, np.uint32), np.zeros((0, 64), _lib.EDIT_OP_DTYPE), 65)
    with pytest.raises(ValueError, match="scripts of shape"):
        hs.move_profile_of_wide(ts, empty, es, host=True)
    with pytest.raises(ValueError, match="scripts of shape"):
        hs.move_profile_of(ts, empty, hs.EditScripts(es.dist, np.zeros((0, 65), _lib.EDIT_OP_DTYPE), 65), host=True)
    assert ctypes.sizeof(ctypes.c_uint32) * 12 == _lib.MOVE_COUNTS_DTYPE.itemsize
