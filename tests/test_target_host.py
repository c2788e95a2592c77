"""CPU: nmz_replayable_target_host (the host decision of the nearest-order sweep, csrc/target.hip) against the numpy
restatement over the C oracle's delays (tests/target_ref.py) and the FNV-only known answers
(tests/golden/target_order_kat.json); historystorage.match_target; argument errors. Everything is integer: every
comparison is equality."""
import functools
import json
import os

import numpy as np
import pytest

import delivery_ref as R
import target_ref as T
from namazu_amd import _lib, historystorage
from namazu_amd.explorepolicy import Replayable

MS = R.MS
NONE = R.NONE


@functools.lru_cache(maxsize=None)
def kat():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "target_order_kat.json")) as f:
        return json.load(f)


# (E, seeds, entities, every k-th event NMZ_NONE): the issue's cases; m = 10^8, decimal seeds from 0
CASES = [(64, 300, 4, 0), (65, 300, 16, 9), (257, 65, 2, 0), (1025, 63, 9, 13)]
M = 10**8


@functools.lru_cache(maxsize=None)
def case(E, S, n_ent, none_every):
    """Inputs, delays and the targets of one case, computed once and shared (not modified): own = seed "1"'s order,
    reverse = that order reversed, random = a random permutation of the events."""
    hints, arrival, _sym, entity = R.case_inputs(E, M, n_ent, none_every)
    seeds = R.decimal_seeds(0, S)
    dl = R.delays(seeds, hints, M)
    own = R.Ref(dl[1:2], arrival, np.zeros(E, np.uint64)).order[0]
    targets = {"own": T.target_of_order(own, E), "reverse": T.target_of_order(own[::-1], E),
               "random": T.target_of_order(np.random.default_rng(E).permutation(E), E)}
    return hints, arrival, entity, seeds, dl, targets


def assert_not_vacuous(ref, kind, min_distinct=8):
    """min_distinct = 8 everywhere but the 8-event PO fixture, whose 7 pairs allow 8 values at the most: 6 there."""
    nd, pl = ref.stats["n_discordant"], ref.stats["prefix_len"]
    if kind == "own":
        assert len(np.unique(nd)) >= min_distinct, "degenerate input: too few distinct n_discordant values"
        assert (nd == 0).any(), "degenerate input: no seed reproduces the target"
        assert len(np.unique(pl)) >= 5, "degenerate input: fewer than 5 distinct prefix_len values"
    else:
        assert int(nd.max()) > ref.n_pairs // 4, "degenerate input: the counts stay small"


@pytest.mark.parametrize("kind", ["own", "reverse", "random"])
@pytest.mark.parametrize("E,S,n_ent,none_every", CASES)
def test_host_equals_the_restatement(E, S, n_ent, none_every, kind):
    hints, arrival, entity, seeds, dl, targets = case(E, S, n_ent, none_every)
    tp = targets[kind]
    for ent in (None, entity):
        ref = T.TRef(dl, arrival, tp, ent)
        assert_not_vacuous(ref, kind)  # from the restatement alone, before any comparison
        got, n_counted, n_pairs = T.host_target(seeds, hints, arrival, ent, tp, M)
        assert (n_counted, n_pairs) == (ref.n_counted, ref.n_pairs)
        assert R.same(got, ref.stats)


@pytest.mark.parametrize("name", ["G", "H"])
def test_host_equals_the_known_answers(name):
    fx = kat()[name]
    seeds = [str(s) for s in range(fx["n_seeds"])]
    ent = fx.get("entity")
    ref = T.TRef(R.delays(seeds, fx["hints"], fx["max_interval_ns"]), fx["arrival_ns"], fx["target_pos"], ent)
    assert_not_vacuous(ref, "own", 8 if name == "G" else 6)
    got, n_counted, n_pairs = T.host_target(seeds, fx["hints"], fx["arrival_ns"], ent, fx["target_pos"],
                                            fx["max_interval_ns"])
    assert (n_counted, n_pairs) == (fx["n_counted"], fx["n_pairs"]) == (ref.n_counted, ref.n_pairs)
    for f in ("n_discordant", "prefix_len", "n_in_place", "min_gap_ns"):
        assert got[f].tolist() == fx[f], f
    assert R.same(got, ref.stats)
    for mode in ("pairs", "prefix"):
        want = fx["top8_" + mode]
        tk = T.topk(got, n_pairs, range(len(seeds)), 8, mode)
        assert [{k: int(e[k]) for k in ("seed", "sum_delay_ns", "n_fault", "first_fault")} for e in tk] == want


def test_zero_discordant_iff_the_order_is_the_target():
    fx = kat()["G"]
    seeds = [str(s) for s in range(fx["n_seeds"])]
    got, _, _ = T.host_target(seeds, fx["hints"], fx["arrival_ns"], None, fx["target_pos"], fx["max_interval_ns"])
    _, order, _ = R.host_delivery(seeds, fx["hints"], fx["arrival_ns"], np.zeros(6, np.uint64), None,
                                  fx["max_interval_ns"])
    equal = (order == np.asarray(fx["target_order"], np.uint32)[None, :]).all(axis=1)
    assert equal.any() and not equal.all()
    assert np.array_equal(got["n_discordant"] == 0, equal)
    assert np.array_equal(got["prefix_len"] == 6, equal) and np.array_equal(got["n_in_place"] == 6, equal)


@pytest.mark.parametrize("E,S,n_ent,none_every", CASES[:2])
def test_the_reverse_target_counts_the_other_pairs(E, S, n_ent, none_every):
    hints, arrival, entity, seeds, _dl, targets = case(E, S, n_ent, none_every)
    for ent in (None, entity):
        a, _, n_pairs = T.host_target(seeds, hints, arrival, ent, targets["own"], M)
        b, _, _ = T.host_target(seeds, hints, arrival, ent, targets["reverse"], M)
        assert np.array_equal(a["n_discordant"].astype(np.int64) + b["n_discordant"], np.full(S, n_pairs))
        assert a["min_gap_ns"].tobytes() == b["min_gap_ns"].tobytes()


def test_absent_and_sparse_target_positions():
    """Every 5th event absent and positions 7 i + 3: the absent events are not counted, and only the order of the
    positions is read."""
    hints, arrival, entity, seeds, dl, targets = case(65, 300, 16, 9)
    own = np.argsort(targets["own"], kind="stable")
    kept = np.array([e for e in own if e % 5 != 4])
    dense, sparse = T.target_of_order(kept, 65), T.target_of_order(kept, 65, stride=7, offset=3)
    for ent in (None, entity):
        ref = T.TRef(dl, arrival, sparse, ent)
        got, n_counted, n_pairs = T.host_target(seeds, hints, arrival, ent, sparse, M)
        assert R.same(got, ref.stats) and (n_counted, n_pairs) == (ref.n_counted, ref.n_pairs)
        assert got.tobytes() == T.host_target(seeds, hints, arrival, ent, dense, M)[0].tobytes()
    assert T.TRef(dl, arrival, sparse, None).n_counted == len(kept)


def test_nothing_counted_and_zero_interval():
    hints, arrival, entity, seeds, _dl, targets = case(64, 300, 4, 0)
    got, n_counted, n_pairs = T.host_target(seeds[:3], hints, arrival, None, np.full(64, NONE, np.uint32), M)
    assert (n_counted, n_pairs) == (0, 0)
    assert got.tolist() == [(0, 0, R.INT64_MAX, NONE, 0)] * 3
    # m == 0: the order is the arrivals' for every seed
    by_arrival = np.lexsort((np.arange(64), arrival))
    got, n_counted, _ = T.host_target(seeds[:3], hints, arrival, None, T.target_of_order(by_arrival, 64), 0)
    assert np.all(got["n_discordant"] == 0) and np.all(got["prefix_len"] == 64) and n_counted == 64


def test_target_distance_is_the_host_entry_point():
    fx = kat()["H"]
    p = Replayable()
    p.MaxInterval, p.Seed = fx["max_interval_ns"], "7"
    st, n_counted, n_pairs = p.target_distance(fx["hints"], fx["arrival_ns"], fx["target_pos"], fx["entity"])
    assert int(st["n_discordant"]) == fx["n_discordant"][7] and int(st["prefix_len"]) == fx["prefix_len"][7]
    assert (n_counted, n_pairs) == (fx["n_counted"], fx["n_pairs"])


def test_match_target():
    # repeated symbols: occurrences pair up in arrival order, ties to the smaller index
    sym = [5, 7, 5, 9, 5]
    arrival = [10, 0, 3, 1, 3]
    tp = historystorage.match_target(sym, arrival, [5, 5, 7, 8, 5, 5])
    assert tp.dtype == np.uint32 and tp.tolist() == [4, 2, 0, NONE, 1]
    # more events than recorded occurrences: the latest arrivals stay unmatched
    assert historystorage.match_target([1, 1, 1], [30, 10, 20], [1, 2, 1]).tolist() == [NONE, 0, 2]
    assert historystorage.match_target([1, 2], [0, 0], []).tolist() == [NONE, NONE]
    assert historystorage.match_target([], [], [1]).tolist() == []
    with pytest.raises(ValueError, match="arrival times"):
        historystorage.match_target([1, 2], [0], [1])
    # distinct symbols: the inverse of the recorded order, whatever the arrivals
    rng = np.random.default_rng(4)
    sym = rng.permutation(2**20)[:50].astype(np.uint64)
    rec = sym[rng.permutation(50)]
    tp = historystorage.match_target(sym, rng.integers(0, 5, 50), rec)
    assert np.array_equal(rec[tp], sym)


def host(hints, arrival, entity, tp, m, n_events=None):
    from oracle import oracle as O
    L = _lib.load()
    ho, hb = O.to_csr(list(hints))
    arr = np.ascontiguousarray(arrival, np.int64)
    t = np.ascontiguousarray(tp, np.uint32)
    en = None if entity is None else np.ascontiguousarray(entity, np.uint32)
    st = np.zeros(1, _lib.TARGET_STATS_DTYPE)
    sb = np.frombuffer(b"1", np.uint8)
    _lib.check(L.nmz_replayable_target_host(_lib.ptr(sb), 1, _lib.ptr(ho), _lib.ptr(hb),
                                            len(hints) if n_events is None else n_events, m, _lib.ptr(arr),
                                            _lib.ptr(en), _lib.ptr(t), _lib.ptr(st), None, None))
    return st[0]


def test_argument_errors():
    hints, arr, tp = ["a", "b", "c"], [0, 1, 2], [0, 1, 2]
    assert int(host(hints, arr, None, tp, 10)["prefix_len"]) <= 3
    with pytest.raises(_lib.NmzInvalidArgument, match="target_pos 1 appears twice among the counted events"):
        host(hints, arr, None, [0, 1, 1], 10)
    # a duplicate on an event that is not counted is legal
    host(hints, arr, [0, 0, NONE], [0, 1, 1], 10)
    with pytest.raises(_lib.NmzInvalidArgument, match=r"n_events must be in \[1, 4096\]"):
        host(hints, arr, None, tp, 10, n_events=0)
    with pytest.raises(_lib.NmzInvalidArgument, match=r"n_events must be in \[1, 4096\]"):
        host(hints, arr, None, tp, 10, n_events=4097)
    with pytest.raises(_lib.NmzInvalidArgument, match=r"max_interval_ns must be in \[0, 2\^50\]"):
        host(hints, arr, None, tp, 2**50 + 1)
    with pytest.raises(_lib.NmzInvalidArgument, match=r"max_interval_ns must be in \[0, 2\^50\]"):
        host(hints, arr, None, tp, -1)
    with pytest.raises(_lib.NmzInvalidArgument, match=r"arrival_ns\[1\] must be in \[0, 2\^50\]"):
        host(hints, [0, 2**50 + 1, 2], None, tp, 10)
    with pytest.raises(_lib.NmzInvalidArgument, match=r"arrival_ns\[2\] must be in \[0, 2\^50\]"):
        host(hints, [0, 1, -2], None, tp, 10)
    with pytest.raises(_lib.NmzInvalidArgument, match=r"entity\[0\] must be < 16384 or NMZ_NONE"):
        host(hints, arr, [16384, 0, 0], tp, 10)
    L = _lib.load()
    st = np.zeros(1, _lib.TARGET_STATS_DTYPE)
    bad_off = np.array([0, 2, 1, 3], np.uint32)
    a, t = np.array(arr, np.int64), np.array(tp, np.uint32)
    hb = np.frombuffer(b"abc", np.uint8)
    rc = L.nmz_replayable_target_host(None, 0, _lib.ptr(bad_off), _lib.ptr(hb), 3, 10, _lib.ptr(a), None, _lib.ptr(t),
                                      _lib.ptr(st), None, None)
    assert rc == _lib.NMZ_EINVAL and "hint offsets must not decrease" in _lib.last_error()
    rc = L.nmz_replayable_target_host(None, 0, _lib.ptr(bad_off), _lib.ptr(hb), 3, 10, _lib.ptr(a), None, None,
                                      _lib.ptr(st), None, None)
    assert rc == _lib.NMZ_EINVAL and "target_pos is NULL" in _lib.last_error()
    # the Python layer: a bad rank mode and a bad target never reach the library
    p = Replayable()
    p.MaxInterval = 10
    with pytest.raises(ValueError, match="rank_by must be one of"):
        p.NearestOrders(hints, arr, target_pos=tp, seed_lo=0, n_seeds=1, rank_by="nearest", ctx=object())
    with pytest.raises(ValueError, match="either target_order or target_pos"):
        p.NearestOrders(hints, arr, seed_lo=0, n_seeds=1, ctx=object())
    with pytest.raises(ValueError, match="holds an event twice"):
        p.NearestOrders(hints, arr, target_order=[0, 0], seed_lo=0, n_seeds=1, ctx=object())
