"""CPU: nmz_replayable_delivery_host (one seed's delivery order, releases and signature on the calling thread)
against the numpy restatement over the C oracle's delays (tests/delivery_ref.py) and the FNV-only known answers of
tests/golden/delivery_order_kat.json. Everything is integer: every comparison is equality."""
import numpy as np
import pytest

import delivery_ref as R
from namazu_amd import _lib
from oracle import oracle as O

MS = R.MS
SEEDS = ["", "foobar"] + [str(i) for i in range(40)]  # the empty seed is the reference's default


def host_one(seed, hints, arrival, sym, entity, m, want=(True, True, True)):
    L = _lib.load()
    ho, hb = O.to_csr(list(hints))
    E = len(hints)
    b = seed.encode()
    sb = np.frombuffer(b, np.uint8) if b else np.zeros(1, np.uint8)
    arr = None if arrival is None else np.ascontiguousarray(arrival, np.int64)
    sy = None if sym is None else np.ascontiguousarray(sym, np.uint64)
    en = None if entity is None else np.ascontiguousarray(entity, np.uint32)
    st = np.zeros(1, _lib.DELIVERY_STATS_DTYPE) if want[0] else None
    order = np.zeros(max(E, 1), np.uint32) if want[1] else None
    rel = np.zeros(max(E, 1), np.int64) if want[2] else None
    _lib.check(L.nmz_replayable_delivery_host(_lib.ptr(sb), len(b), _lib.ptr(ho), _lib.ptr(hb), E, m, _lib.ptr(arr),
                                              _lib.ptr(sy), _lib.ptr(en), _lib.ptr(st), _lib.ptr(order),
                                              _lib.ptr(rel)))
    return (st[0] if want[0] else None), order, rel


@pytest.mark.parametrize("m", [0, 1, 7, 2**31 - 1, 2**31, 2**32 + 5, 2**50])
@pytest.mark.parametrize("E,n_ent,none_every", [(1, 0, 0), (2, 1, 0), (65, 0, 0), (65, 7, 5), (300, 70, 9)])
def test_against_restatement(m, E, n_ent, none_every):
    hints, arrival, sym, entity = R.case_inputs(E, m, n_ent, none_every)
    ref = R.Ref(R.delays(SEEDS, hints, m), arrival, sym, entity)
    st, order, rel = R.host_delivery(SEEDS, hints, arrival, sym, entity, m)
    assert np.array_equal(rel, ref.release)
    G = ref.order.shape[1]
    assert np.array_equal(order[:, :G], ref.order) and np.all(order[:, G:] == R.NONE)
    assert R.same(st, ref.stats)


def test_ties_go_by_event_index():
    hints = ["same", "same", "same", "other", "other"]
    sym = np.arange(5, dtype=np.uint64) + np.uint64(100)
    # equal hints with equal arrivals: equal releases for every seed, delivered in index order, a gap of 0
    for seed in SEEDS[:8]:
        st, order, rel = host_one(seed, hints, [5, 5, 5, 10**9, 10**9], sym, None, 10**8)
        assert rel[0] == rel[1] == rel[2] and rel[3] == rel[4]
        pos = {int(e): i for i, e in enumerate(order)}
        assert pos[0] < pos[1] < pos[2] and pos[3] < pos[4]
        assert st["min_gap_ns"] == 0 and st["gap_event"] == 1 and st["n_counted"] == 5
    # m == 0 with equal arrivals: the order is (arrival, index)
    st, order, rel = host_one("x", ["a", "b", "c", "d"], [7, 3, 7, 3], sym[:4], None, 0)
    assert order.tolist() == [1, 3, 0, 2] and rel.tolist() == [7, 3, 7, 3]
    assert st["min_gap_ns"] == 0 and st["gap_event"] == 2  # pairs (1,3) and (0,2) tie at 0: later events 3 and 2
    # m == 1: every delay is 0
    st1, order1, rel1 = host_one("y", ["a", "b", "c", "d"], [7, 3, 7, 3], sym[:4], None, 1)
    assert order1.tolist() == [1, 3, 0, 2] and rel1.tolist() == [7, 3, 7, 3] and st1 == st


def test_none_events_are_skipped_and_single_event_entities_give_no_gap():
    hints = [f"h{i}" for i in range(6)]
    sym = np.arange(6, dtype=np.uint64)
    arrival = [0, MS, 2 * MS, 3 * MS, 4 * MS, 5 * MS]
    ent = [0, R.NONE, 1, R.NONE, 2, R.NONE]
    st, order, rel = host_one("1", hints, arrival, sym, ent, 1000)
    assert st["n_counted"] == 3 and order[:3].tolist() == [0, 2, 4] and np.all(order[3:] == R.NONE)
    assert st["min_gap_ns"] == R.INT64_MAX and st["gap_event"] == R.NONE  # one event per entity: no pair compared
    assert len(rel) == 6 and np.all(rel >= np.array(arrival))            # releases of the skipped events too
    # the skipped events do not enter the signature: the same as the trace without them
    st2, _, _ = host_one("1", hints[::2], arrival[::2], sym[::2], [0, 1, 2], 1000)
    assert (st2["sig_lo"], st2["sig_hi"]) == (st["sig_lo"], st["sig_hi"])
    # nothing counted
    st3, order3, _ = host_one("1", hints, arrival, sym, [R.NONE] * 6, 1000)
    assert st3["n_counted"] == 0 and np.all(order3 == R.NONE) and st3["min_gap_ns"] == R.INT64_MAX
    # one entity for all events == exact mode
    a = host_one("5", hints, arrival, sym, [3] * 6, 4 * MS)[0]
    b = host_one("5", hints, arrival, sym, None, 4 * MS)[0]
    assert a == b and a["min_gap_ns"] < R.INT64_MAX
    # optional outputs
    assert host_one("5", hints, arrival, sym, None, 4 * MS, want=(False, False, False)) == (None, None, None)


def test_limits():
    hints = ["a", "b", "c"]
    sym = np.arange(3, dtype=np.uint64)
    arr = [0, 1, 2]

    def bad(match, **kw):
        a = dict(seed="s", hints=hints, arrival=arr, sym=sym, entity=None, m=10)
        a.update(kw)
        with pytest.raises(_lib.NmzInvalidArgument, match=match):
            host_one(a["seed"], a["hints"], a["arrival"], a["sym"], a["entity"], a["m"])

    bad(r"n_events must be in \[1, 4096\]", hints=[], arrival=[], sym=sym[:0])
    big = ["h"] * 4097
    bad(r"n_events must be in \[1, 4096\]", hints=big, arrival=[0] * 4097, sym=np.zeros(4097, np.uint64))
    bad(r"max_interval_ns must be in \[0, 2\^50\]", m=-1)
    bad(r"max_interval_ns must be in \[0, 2\^50\]", m=2**50 + 1)
    bad(r"arrival_ns\[1\] must be in \[0, 2\^50\]", arrival=[0, -1, 2])
    bad(r"arrival_ns\[2\] must be in \[0, 2\^50\]", arrival=[0, 1, 2**50 + 1])
    bad(r"entity\[1\] must be < 16384 or NMZ_NONE", entity=[0, 16384, 1])
    bad("NULL", sym=None)
    bad("NULL", arrival=None)
    # the limits themselves are legal
    st, _, _ = host_one("s", hints, [0, 2**50, 5], sym, [16383, R.NONE, 0], 2**50)
    assert st["n_counted"] == 2
    assert host_one("s", ["h"] * 4096, [0] * 4096, np.zeros(4096, np.uint64), None, 3)[0]["n_counted"] == 4096
    # hint offsets must not decrease; seed NULL with a length
    L = _lib.load()
    off = np.array([0, 2, 1, 3], np.uint32)
    hb = np.frombuffer(b"abc", np.uint8)
    a64 = np.zeros(3, np.int64)
    assert L.nmz_replayable_delivery_host(None, 0, _lib.ptr(off), _lib.ptr(hb), 3, 10, _lib.ptr(a64), _lib.ptr(sym),
                                          None, None, None, None) == _lib.NMZ_EINVAL
    assert "hint offsets must not decrease" in _lib.last_error()
    off = np.array([0, 1, 2, 3], np.uint32)
    assert L.nmz_replayable_delivery_host(None, 3, _lib.ptr(off), _lib.ptr(hb), 3, 10, _lib.ptr(a64), _lib.ptr(sym),
                                          None, None, None, None) == _lib.NMZ_EINVAL
    assert "seed is NULL" in _lib.last_error()
    # the device entry points reject a NULL context or plan before any device work
    assert L.nmz_replayable_delivery_sweep_decimal(None, 0, 1, _lib.ptr(off), _lib.ptr(hb), 3, 10, _lib.ptr(a64),
                                                   _lib.ptr(sym), None, None, None, None, None) == _lib.NMZ_EINVAL
    assert "ctx is NULL" in _lib.last_error()
    assert L.nmz_replayable_delivery_sweep_decimal_dev(None, 0, 1, None, None) == _lib.NMZ_EINVAL
    assert L.nmz_delivery_classes_dev(None, None, 0, None, None, None, None) == _lib.NMZ_EINVAL
    assert L.nmz_sig_classes_dev(None, None, 0, None, None) == _lib.NMZ_EINVAL
    assert L.nmz_replayable_delivery_plan_destroy(None) == _lib.NMZ_OK


def kat_classes(fx, m, entity=None):
    seeds = [str(s) for s in range(fx["n_seeds"])]
    st, order, rel = R.host_delivery(seeds, fx["hints"], fx["arrival_ns"], fx["sym"], entity, m)
    sig = list(zip(st["sig_lo"].tolist(), st["sig_hi"].tolist()))
    first = {}
    fe = np.array([first.setdefault(s, i) for i, s in enumerate(sig)])
    return seeds, st, order, fe


def test_known_answers_fixture_G(golden):
    fx = golden("delivery_order_kat.json")["G"]
    # under the 1 ms spacing no release overtakes: every seed delivers the identity order
    seeds, st, order, fe = kat_classes(fx, 2**19)
    assert np.all(fe == 0) and np.all(order == np.arange(6)) and np.all(st["min_gap_ns"] >= MS - 2**19)
    seeds, st, order, fe = kat_classes(fx, 0)
    assert np.all(fe == 0) and np.all(order == np.arange(6)) and np.all(st["min_gap_ns"] == MS)
    assert np.all(st["gap_event"] == 1)
    # 6 ms: the classes recorded by the FNV-only script
    seeds, st, order, fe = kat_classes(fx, fx["max_interval_ns"])
    ex = fx["exact"]
    R.assert_partition_mixed(np.array([int(h["seed"]) for h in ex["heads"] for _ in range(h["size"])]))
    heads = np.nonzero(fe == np.arange(len(fe)))[0]
    sizes = R.class_sizes(fe)
    assert len(heads) == ex["n_classes"] == 146 and sizes.max() == ex["largest_class"]
    assert (sizes >= 2).sum() == ex["n_merged"] == 80 and (sizes == 1).sum() == ex["n_singletons"] == 66
    for h, w in zip(heads, ex["heads"]):
        assert seeds[h] == w["seed"] and order[h].tolist() == w["order"] and sizes[h] == w["size"]


def test_known_answers_fixture_H(golden):
    fx = golden("delivery_order_kat.json")["H"]
    seeds, st, order, fe = kat_classes(fx, fx["max_interval_ns"])
    ex = fx["exact"]
    R.assert_partition_mixed(np.array([int(h["seed"]) for h in ex["heads"] for _ in range(h["size"])]))
    heads = np.nonzero(fe == np.arange(len(fe)))[0]
    sizes = R.class_sizes(fe)
    assert len(heads) == ex["n_classes"] == 344 and sizes.max() == ex["largest_class"]
    for h, w in zip(heads, ex["heads"]):
        assert seeds[h] == w["seed"] and order[h].tolist() == w["order"] and sizes[h] == w["size"]
    # per-entity orders: 8 classes, none a singleton
    seeds, st, order, fe = kat_classes(fx, fx["max_interval_ns"], fx["entity"])
    po = fx["po"]
    R.assert_partition_mixed(np.array([int(h["seed"]) for h in po["heads"] for _ in range(h["size"])]),
                             singletons=False)
    heads = np.nonzero(fe == np.arange(len(fe)))[0]
    sizes = R.class_sizes(fe)
    assert len(heads) == po["n_classes"] == 8 and sizes.max() == po["largest_class"]
    assert [(seeds[h], int(sizes[h])) for h in heads] == [(w["seed"], w["size"]) for w in po["heads"]]
