"""The Python mirror of the delivery sweep: DeliveryResult.representatives and replay.distinct_order_seeds on
hand-made results and Replayable.delivery_order on the host (CPU), and Replayable.DeliveryOrders ->
representatives -> distinct_order_seeds -> replay_env end to end (GPU)."""
import numpy as np
import pytest

import delivery_ref as R
from namazu_amd import _lib, historystorage, replay
from namazu_amd.explorepolicy import DeliveryResult, Replayable

NONE = _lib.NMZ_NONE


def hand_made():
    """Six seeds in three classes: {0, 2, 5} (rep 2, gap 90), {1, 4} (rep 1: a gap tie goes to the smaller index),
    {3} (gap 3)."""
    st = np.zeros(6, _lib.DELIVERY_STATS_DTYPE)
    st["sig_lo"] = [10, 20, 10, 30, 20, 10]
    st["sig_hi"] = [11, 21, 11, 31, 21, 11]
    st["min_gap_ns"] = [50, 70, 90, 3, 70, 60]
    first = np.array([0, 1, 0, 3, 1, 0], np.uint32)
    rep = np.array([2, 1, NONE, 3, NONE, NONE], np.uint32)
    return DeliveryResult(st, first, rep, 3)


def test_representatives_filtering():
    r = hand_made()
    assert r.representatives() == [2, 1, 3]
    assert r.representatives(min_gap_ns=4) == [2, 1]
    assert r.representatives(min_gap_ns=71) == [2]
    assert r.representatives(min_gap_ns=91) == []
    assert r.representatives(known_sigs=[(20, 21)]) == [2, 3]
    assert r.representatives(known_sigs=np.array([[10, 11], [30, 31], [99, 98]], np.uint64)) == [1]
    assert r.representatives(known_sigs=[(10, 21)]) == [2, 1, 3]  # both words must match
    assert r.representatives(min_gap_ns=60, known_sigs=[(10, 11)]) == [1]
    assert r.representatives(known_sigs=np.zeros((0, 2), np.uint64)) == [2, 1, 3]


def test_distinct_order_seeds_to_replay_env():
    r = hand_made()
    seeds = ["s0", b"s1", "s2", "s3", "s4", "s5"]
    assert replay.distinct_order_seeds(r, seeds) == ["s2", "s1", "s3"]
    assert replay.distinct_order_seeds(r, seeds, min_gap_ns=4, known_sigs=[(10, 11)]) == ["s1"]
    assert replay.distinct_order_seeds(r, range(1000, 1006)) == ["1002", "1001", "1003"]  # a decimal sweep
    env = replay.replay_env(replay.distinct_order_seeds(r, seeds)[0], {"PATH": "/bin"})
    assert env == {"PATH": "/bin", replay.REPLAY_SEED_ENV: "s2"}


def test_delivery_order_on_the_host():
    p = Replayable()
    p.MaxInterval = 10**8
    p.Seed = "1029"
    hints, arrival, sym, entity = R.case_inputs(40, 10**8, 4, 6)
    for ent in (None, entity):
        order, rel, st = p.delivery_order(hints, arrival, sym, ent)
        ref = R.Ref(R.delays([p.Seed], hints, p.MaxInterval), arrival, sym, ent)
        assert np.array_equal(order, ref.order[0]) and np.array_equal(rel, ref.release[0])
        assert st.tobytes() == ref.stats[0].tobytes() and len(order) == st["n_counted"]
    p.Seed = ""  # the reference's default seed
    order, rel, st = p.delivery_order(hints, arrival, sym)
    assert np.array_equal(order, R.Ref(R.delays([""], hints, 10**8), arrival, sym).order[0])
    with pytest.raises(ValueError, match="arrival times"):
        p.delivery_order(hints, arrival[:-1], sym)
    for kw in ({}, {"seed_lo": 0}, {"n_seeds": 4}, {"seeds": ["a"], "seed_lo": 0}, {"seeds": ["a"], "n_seeds": 1}):
        with pytest.raises(ValueError, match="either seeds or seed_lo and n_seeds"):  # before any device work
            p.DeliveryOrders(hints, arrival, sym, ctx=object(), **kw)
    with pytest.raises(ValueError, match="entity ids"):
        p.delivery_order(hints, arrival, sym, entity[:-1])


@pytest.mark.gpu
def test_delivery_orders_to_replay_seeds(ctx, golden):
    fx = golden("delivery_order_kat.json")["G"]
    p = Replayable()
    p.MaxInterval = fx["max_interval_ns"]
    seeds = [str(s) for s in range(fx["n_seeds"])]
    r = p.DeliveryOrders(fx["hints"], fx["arrival_ns"], fx["sym"], seeds=seeds, ctx=ctx)
    ref = R.Ref(R.delays(seeds, fx["hints"], p.MaxInterval), fx["arrival_ns"], fx["sym"])
    R.assert_partition_mixed(ref.first_equal())
    assert r.n_classes == fx["exact"]["n_classes"] and np.array_equal(r.class_rep, ref.class_rep())
    reps = r.representatives()
    heads = np.nonzero(ref.first_equal() == np.arange(len(seeds)))[0]
    assert reps == [int(ref.class_rep()[h]) for h in heads] and len(reps) == 146
    # a margin drops the classes whose best member is still too tight; recorded runs drop theirs
    tight = r.representatives(min_gap_ns=200_000)
    assert 0 < len(tight) < len(reps) and all(r.stats["min_gap_ns"][i] >= 200_000 for i in tight)
    assert set(tight) == {i for i in reps if ref.stats["min_gap_ns"][i] >= 200_000}
    # stored runs that delivered the orders of seeds 0 and 17: their signatures through historystorage
    recorded = [historystorage.SingleTrace(np.asarray(fx["sym"], np.uint64)[ref.order[s]],
                                           action_symbols=np.asarray(fx["sym"], np.uint64)[ref.order[s]])
                for s in (0, 17)]
    known = historystorage.trace_signatures(recorded, po_reduction=False, ctx=ctx)
    assert known.shape == (2, 2)
    assert (int(known[1][0]), int(known[1][1])) == (int(r.stats["sig_lo"][17]), int(r.stats["sig_hi"][17]))
    out = replay.distinct_order_seeds(r, seeds, known_sigs=known)
    gone = {int(ref.first_equal()[0]), int(ref.first_equal()[17])}
    assert len(out) == 146 - len(gone)
    assert out == [seeds[i] for i in reps if int(ref.first_equal()[i]) not in gone]
    assert replay.replay_env(out[0])[replay.REPLAY_SEED_ENV] == out[0]
    # the decimal form gives the same result
    r2 = p.DeliveryOrders(fx["hints"], fx["arrival_ns"], fx["sym"], seed_lo=0, n_seeds=len(seeds), ctx=ctx)
    assert r2.stats.tobytes() == r.stats.tobytes() and np.array_equal(r2.class_rep, r.class_rep)
