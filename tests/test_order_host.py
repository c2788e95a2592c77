"""CPU: nmz_replayable_order_host (one seed against event-order constraints, no GPU) against the numpy restatement
over the C oracle's delays (tests/order_ref.py) and the known answers of tests/golden/order_sweep_kat.json."""
import ctypes

import numpy as np
import pytest

import order_ref as R
from namazu_amd import _lib
from namazu_amd.explorepolicy import Replayable
from oracle import oracle as O

MS = R.MS
F_SEEDS = R.decimal_seeds(0, 4096)[0]


def host_fixture(m):
    return R.host_order(F_SEEDS, R.F_HINTS, R.F_ARRIVAL, R.F_CONS, m)


def test_kat_file_describes_the_fixture(golden):
    kat = golden("order_sweep_kat.json")
    assert [tuple(p) for p in kat["pairs_as_listed"]] == list(R.F_PAIRS)
    assert [tuple(c) for c in kat["constraints_before_after_margin"]] == list(R.F_CONS)
    assert kat["n_events"] == len(R.F_HINTS) and kat["n_seeds"] == len(F_SEEDS)
    assert [kat["hint_format"].replace("{i%4}", str(i % 4)).replace("{i}", str(i)) for i in range(16)] == \
        list(R.F_HINTS)
    assert [i * kat["arrival_step_ns"] for i in range(16)] == list(R.F_ARRIVAL)


@pytest.mark.parametrize("m", [10**8, 9 * 10**9, 2**20])
def test_fixture_matches_restatement_and_kat(golden, m):
    st, sl = host_fixture(m)
    exp = R.fixture_stats(m)
    assert R.same(st, exp)
    assert np.array_equal(sl, R.slacks(R.delays(F_SEEDS, R.F_HINTS, m), R.F_ARRIVAL, R.F_CONS))
    case = golden("order_sweep_kat.json")["cases"][str(m)]
    hist = np.bincount(st["n_satisfied"], minlength=6).tolist()
    if "n_satisfied_histogram" in case:
        assert hist == case["n_satisfied_histogram"]
    if "n_all_satisfied" in case:
        assert hist[5] == case["n_all_satisfied"]
        assert int((st["sat_mask"] == 0b11111).sum()) == case["n_all_satisfied"]
    if "argmin_constraint_everywhere" in case:
        assert np.all(st["argmin_constraint"] == case["argmin_constraint_everywhere"])
    if "top" in case:
        top = R.topk(st, np.arange(4096, dtype=np.uint64), len(case["top"]))
        for got, want in zip(top, case["top"]):
            assert (int(got["seed"]), int(got["n_fault"]), int(got["sum_delay_ns"]), int(got["first_fault"])) == \
                (want["seed"], want["n_satisfied"], want["min_slack_ns"], want["argmin_constraint"])
        # both outcomes are present: seeds that satisfy everything and seeds that satisfy nothing
        assert hist[0] > 0 and hist[5] > 0


SEEDS = R.SEEDS  # starts with the empty seed, the reference's default


@pytest.mark.parametrize("m", R.M_CASES)
def test_moduli(m):
    st, sl = R.host_order(SEEDS, R.F_HINTS, R.F_ARRIVAL, R.F_CONS, m)
    dl = R.delays(SEEDS, R.F_HINTS, m)
    assert R.same(st, R.stats_from_slack(R.slacks(dl, R.F_ARRIVAL, R.F_CONS)))
    assert np.array_equal(sl, R.slacks(dl, R.F_ARRIVAL, R.F_CONS))
    if m <= 1:  # every delay is 0: the slack does not depend on the seed
        assert np.all(sl == sl[0]) and np.array_equal(sl[0], [-26 * MS, -36 * MS, -5 * MS - 1, -35 * MS, -65 * MS - 1])


def test_interval_is_the_oracles():
    """One decision spelled out: the slack is built from oracle.replayable_interval of the two events."""
    m = 10**8
    _, sl = R.host_order(["foobar"], R.F_HINTS, R.F_ARRIVAL, [(12, 7, 10 * MS)], m)
    d = [O.replayable_interval("foobar", R.F_HINTS[e], m) for e in (7, 12)]
    assert sl[0, 0] == (R.F_ARRIVAL[7] + d[0]) - (R.F_ARRIVAL[12] + d[1]) - 10 * MS


def test_empty_hint():
    hints = list(R.F_HINTS)
    hints[5] = ""
    for m in (10**8, 9 * 10**9):
        st, _ = R.host_order(SEEDS, hints, R.F_ARRIVAL, R.F_CONS, m)
        assert R.same(st, R.stats(SEEDS, hints, R.F_ARRIVAL, R.F_CONS, m))


def test_equal_hints_slack_is_the_same_for_every_seed():
    hints = ["same", "other", "same", ""]
    arrival = [0, 1, 7 * MS, 9 * MS]
    st, sl = R.host_order(SEEDS, hints, arrival, [(0, 2, MS), (2, 0, MS)], 10**8)
    assert np.all(sl[:, 0] == 6 * MS) and np.all(sl[:, 1] == -8 * MS)
    assert np.all(st["sat_mask"] == 1) and np.all(st["n_satisfied"] == 1)
    assert np.all(st["min_slack_ns"] == -8 * MS) and np.all(st["argmin_constraint"] == 1)


def test_equal_slack_argmin_is_the_first():
    cons = [(9, 2, 1), (5, 0, MS), (5, 0, MS), (9, 2, 1)]
    st, sl = R.host_order(SEEDS, R.F_HINTS, R.F_ARRIVAL, cons, 10**8)
    assert np.array_equal(sl[:, 0], sl[:, 3]) and np.array_equal(sl[:, 1], sl[:, 2])
    assert set(st["argmin_constraint"].tolist()) == {0, 1}  # never the later twin; both first twins occur
    assert R.same(st, R.stats(SEEDS, R.F_HINTS, R.F_ARRIVAL, cons, 10**8))


def test_one_and_sixty_four_constraints():
    st, _ = R.host_order(SEEDS, R.F_HINTS, R.F_ARRIVAL, R.F_CONS[:1], 10**8)
    assert R.same(st, R.stats(SEEDS, R.F_HINTS, R.F_ARRIVAL, R.F_CONS[:1], 10**8))
    assert set(st["sat_mask"].tolist()) == {0, 1} and np.all(st["argmin_constraint"] == 0)
    hints, arrival, cons = R.wide_constraints()
    st, _ = R.host_order(SEEDS, hints, arrival, cons, 10**8)
    assert R.same(st, R.stats(SEEDS, hints, arrival, cons, 10**8))
    assert np.all(st["sat_mask"] >> np.uint64(63) == 1)
    assert len(set(st["sat_mask"].tolist())) > 1


BIG = 2**61
EINVAL_CASES = [
    # (what changes, message fragment)
    (dict(cons=[]), "n_constraints must be in [1, 64]"),
    (dict(cons=[(5, 0, 1)] * 65), "n_constraints must be in [1, 64]"),
    (dict(cons=[(5, 0, 1), (3, 3, 1)]), "constraint 1: before == after"),
    (dict(cons=[(16, 0, 1)]), "constraint 0: event index out of range"),
    (dict(cons=[(5, 0, 1), (5, 0, 1), (0, 16, 1)]), "constraint 2: event index out of range"),
    (dict(arrival={4: -1}), "arrival_ns[4] must be in [0, 2^61]"),
    (dict(arrival={15: BIG + 1}), "arrival_ns[15] must be in [0, 2^61]"),
    (dict(cons=[(5, 0, 0)]), "constraint 0: margin_ns must be in [1, 2^61]"),
    (dict(cons=[(5, 0, -7)]), "constraint 0: margin_ns must be in [1, 2^61]"),
    (dict(cons=[(5, 0, BIG + 1)]), "constraint 0: margin_ns must be in [1, 2^61]"),
    (dict(m=-1), "max_interval_ns must be in [0, 2^61]"),
    (dict(m=BIG + 1), "max_interval_ns must be in [0, 2^61]"),
]


@pytest.mark.parametrize("change,message", EINVAL_CASES)
def test_limits_are_einval_with_a_message(change, message):
    arrival = list(R.F_ARRIVAL)
    for i, v in change.get("arrival", {}).items():
        arrival[i] = v
    with pytest.raises(_lib.NmzInvalidArgument) as e:
        R.host_order(["7"], R.F_HINTS, arrival, change.get("cons", list(R.F_CONS)), change.get("m", 10**8))
    assert e.value.code == _lib.NMZ_EINVAL and message in str(e.value)


def test_limits_are_inclusive():
    """2^61 itself is legal for the arrivals, the margin and the modulus, and the slack still fits int64."""
    arrival = [0, BIG]
    st, sl = R.host_order(SEEDS, ["a", "b"], arrival, [(1, 0, BIG), (0, 1, 1)], BIG)
    dl = R.delays(SEEDS, ["a", "b"], BIG)
    assert np.array_equal(sl, R.slacks(dl, arrival, [(1, 0, BIG), (0, 1, 1)]))
    assert sl.min() >= -3 * BIG and sl.max() <= 2 * BIG and np.all(st["min_slack_ns"] == sl[:, 0])


def test_python_surface():
    p = Replayable()
    p.MaxInterval, p.Seed = 10**8, "1029"
    st, sl = p.order_slack(R.F_HINTS, R.F_ARRIVAL, list(R.F_CONS))
    assert (int(st["n_satisfied"]), int(st["min_slack_ns"]), int(st["argmin_constraint"]), int(st["sat_mask"])) == \
        (5, 3735120, 4, 31)
    assert sl.dtype == np.int64 and sl.shape == (5,) and sl.min() == 3735120 and sl.argmin() == 4
    # tuples, lists and a prepared array are the same constraints
    arr = Replayable.order_constraints([list(c) for c in R.F_CONS])
    assert arr.dtype == _lib.ORDER_CONSTRAINT_DTYPE and arr.dtype.itemsize == 16
    assert [tuple(int(x) for x in c) for c in arr] == list(R.F_CONS)
    assert np.array_equal(p.order_slack(R.F_HINTS, R.F_ARRIVAL, arr)[1], sl)
    p.Seed = ""  # the reference's default seed
    assert np.array_equal(p.order_slack(R.F_HINTS, R.F_ARRIVAL, R.F_CONS)[1],
                          R.host_order([""], R.F_HINTS, R.F_ARRIVAL, R.F_CONS, 10**8)[1][0])
    with pytest.raises(ValueError, match="expected \\(before, after, margin_ns\\)"):
        Replayable.order_constraints([(1, 2)])
    with pytest.raises(ValueError, match="does not fit"):
        Replayable.order_constraints([(-1, 2, 5)])
    with pytest.raises(ValueError, match="arrival times"):
        p.order_slack(R.F_HINTS, R.F_ARRIVAL[:3], R.F_CONS)
    with pytest.raises(_lib.NmzInvalidArgument, match="before == after"):
        p.order_slack(R.F_HINTS, R.F_ARRIVAL, [(2, 2, 1)])
    assert _lib.ORDER_STATS_DTYPE.itemsize == 24
    assert list(_lib.ORDER_STATS_DTYPE.names) == ["sat_mask", "min_slack_ns", "n_satisfied", "argmin_constraint"]


def test_stats_and_slack_may_be_null():
    L = _lib.load()
    ho, hb = O.to_csr(list(R.F_HINTS))
    arr = np.array(R.F_ARRIVAL, np.int64)
    cs = Replayable.order_constraints(R.F_CONS)
    sb = np.frombuffer(b"1029", np.uint8)
    st = np.zeros(1, _lib.ORDER_STATS_DTYPE)
    _lib.check(L.nmz_replayable_order_host(_lib.ptr(sb), 4, _lib.ptr(ho), _lib.ptr(hb), 16, 10**8, _lib.ptr(arr),
                                           _lib.ptr(cs), 5, _lib.ptr(st), None))
    assert int(st[0]["min_slack_ns"]) == 3735120
    _lib.check(L.nmz_replayable_order_host(_lib.ptr(sb), 4, _lib.ptr(ho), _lib.ptr(hb), 16, 10**8, _lib.ptr(arr),
                                           _lib.ptr(cs), 5, None, None))
    assert L.nmz_abi_version() == 1 and ctypes.sizeof(ctypes.c_void_p) == 8
