"""Long and non-ASCII replay hints on the host: the hint families of tests/hint_cases.py have the properties they
are there for, the plain reference of the delays agrees with its Python-integer form and with the C oracle (delays and
full statistics, which licenses the GPU tests to compare with the oracle's records), and the library's host forms --
online decisions, order slack, delivery order, distance to a recorded order -- give the reference's numbers on them.
Everything is an integer and compared with equality."""
import numpy as np
import pytest

import delivery_ref as DR
import hint_cases as H
import order_ref as OR
import target_ref as TR
from namazu_amd import _lib
from oracle import oracle as O


# ---------------------------------------------------------------- the families' properties
def test_seeds():
    s = H.seeds()
    assert len(s) == 300 and s[:256] == [str(i).encode() for i in range(256)]
    assert s[256:260] == [b"", b"foobar", b"\xff" * 7, b"\x00"]
    assert all(len(x) <= 24 for x in s[260:]) and any(b >= 0x80 for x in s[260:] for b in x)
    assert [s[i] for i in H.DECIDE_SEEDS][1:5] == [b"", b"foobar", b"\xff" * 7, b"\x00"]


@pytest.mark.parametrize("r", [1, 2, 3, 0])
def test_joints_properties(r):
    """Every class of 12 holds every start alignment twice, the special byte values occur at every length, the total
    is r (mod 4) behind a non-empty last hint; the 1,000-byte class (12 > WT_BRUTE events) takes the fused reader
    through 63 rounds."""
    hints = H.joints() if r == 1 else H.joints_tail(r)
    assert H.check_joints(hints, r) == 63
    sizes = H.class_sizes(hints)
    assert sizes[1000] == 12 and all(sizes[ln] == 5 for ln in H.JOINT_SMALL)
    assert 380 <= len(hints) <= 560 and 29_000 <= sum(len(h) for h in hints) <= 31_000
    if r != 1:  # the same trace but for its last hint
        base = H.joints()
        assert hints[:-1] == base[:-1] and hints[-1][:len(base[-1])] == base[-1]
        assert len(hints[-1]) - len(base[-1]) == (r - 1) & 3


@pytest.mark.parametrize("E", [5, 300])
@pytest.mark.parametrize("extra", [0, 1])
def test_one_long_properties(E, extra):
    """extra = 1 is the first length past plan_create's counting sort; extra = 0 the last one inside it."""
    hints = H.one_long(E, extra)
    assert len(hints) == E and max(len(h) for h in hints) == 4 * E + 4096 + extra
    assert sorted(len(h) for h in hints)[-2] <= 30 and min(len(h) for h in hints) >= 3
    assert H.takes_comparison_sort(hints) == (extra == 1)


def test_class_structure_properties():
    assert H.class_sizes(H.many_classes()) == {ln: 1 for ln in range(700)}
    assert H.class_sizes(H.mid_classes()) == {ln: 9 for ln in range(10, 190, 2)} and 9 > H.WT_BRUTE
    assert len(H.class_sizes(H.mid_classes())) == 90
    assert H.class_sizes(H.long_class()) == {64: 4097}
    assert len(set(H.long_class())) == 4097
    for name in ("many_classes", "mid_classes"):
        lens = [len(h) for h in H.FAMILIES[name]()]
        assert lens != sorted(lens), f"{name} is not shuffled"


# ---------------------------------------------------------------- the reference against itself and the oracle
@pytest.mark.parametrize("name", sorted(H.FAMILIES))
def test_reference_equals_python_integers(name):
    hints, seeds = H.FAMILIES[name](), H.seeds()[:3]
    for m in (10**8, 2**63 - 1, 0, -1):
        got, exp = H.reference_delays(seeds, hints, m), H.reference_delays_py(seeds, hints, m)
        assert np.array_equal(got, exp), (m, H.first_difference(got, exp, hints))


def test_reference_stats_first_maximum():
    d = np.array([[3, 9, 9, 1], [-1, -5, -1, -7], [2**63 - 1, 0, 2**63 - 1, 5]], np.int64)
    st = H.reference_stats(d)
    assert st["argmax_event"].tolist() == [1, 0, 0] and st["max_delay_ns"].tolist() == [9, -1, 2**63 - 1]
    assert st["sum_delay_ns"].tolist() == [22, 2**64 - 14, (2**64 - 2 + 5) % 2**64]


@pytest.mark.parametrize("name", sorted(H.FAMILIES))
def test_reference_equals_oracle(name):
    """Delays of every seed and the oracle's statistics, at every modulus: the GPU tests may then take the oracle's
    full statistics records as the reference's."""
    hints, seeds = H.FAMILIES[name](), H.family_seeds(name)
    so, sb = O.to_csr(seeds)
    ho, hb = O.to_csr(hints)
    for m in H.M_ALL:
        ref = H.reference_delays(seeds, hints, m)
        st, dl = O.replayable_sweep(so, sb, ho, hb, m, n_dump=len(seeds))
        assert np.array_equal(dl, ref), (m, H.first_difference(dl, ref, hints))
        rs = H.reference_stats(ref)
        for f in rs.dtype.names:
            assert np.array_equal(st[f], rs[f]), (m, f)
        assert not st["n_fault"].any() and (st["first_fault"] == H.NONE).all() and not st["flags"].any()


# ---------------------------------------------------------------- the library's host forms
@pytest.mark.parametrize("name", ["joints", "one_long_5_1"])
def test_decide_host(name):
    """nmz_replayable_decide_host, every seed of seeds()."""
    L = _lib.load()
    hints, seeds = H.FAMILIES[name](), H.seeds()
    ho, hb = O.to_csr(hints)
    for m in (10**8, 2**63 - 1, 0):
        ref = H.reference_delays(seeds, hints, m)
        got = np.zeros_like(ref)
        for i, s in enumerate(seeds):
            sb = np.frombuffer(s, np.uint8) if s else np.zeros(1, np.uint8)
            _lib.check(L.nmz_replayable_decide_host(_lib.ptr(sb), len(s), _lib.ptr(ho), _lib.ptr(hb), len(hints), m,
                                                    _lib.ptr(got[i])))
        assert np.array_equal(got, ref), (m, H.first_difference(got, ref, hints))


def test_order_host():
    hints, seeds = H.joints(), H.host_sweep_seeds()
    cons, arrival = H.order_constraints(hints), np.zeros(len(hints), np.int64)
    sl = OR.slacks(H.reference_delays(seeds, hints, H.HOST_M), arrival, cons)
    st, hsl = OR.host_order(seeds, hints, arrival, cons, H.HOST_M)
    assert np.array_equal(hsl, sl)
    assert OR.same(st, OR.stats_from_slack(sl))


def test_delivery_host():
    hints, seeds = H.joints(), H.host_sweep_seeds()
    _, arrival, sym, _ = DR.case_inputs(len(hints), H.HOST_M)
    dl = H.reference_delays(seeds, hints, H.HOST_M)
    ref = DR.Ref(dl, arrival, sym)
    st, order, rel = DR.host_delivery(seeds, hints, arrival, sym, None, H.HOST_M)
    assert np.array_equal(rel, ref.release), H.first_difference(rel - arrival, dl, hints)
    assert np.array_equal(order, ref.order)
    assert DR.same(st, ref.stats)


def test_target_host():
    hints, seeds = H.joints(), H.host_sweep_seeds()
    _, arrival, sym, _ = DR.case_inputs(len(hints), H.HOST_M)
    dl = H.reference_delays(seeds, hints, H.HOST_M)
    tp = TR.target_of_order(DR.Ref(dl[1:2], arrival, sym).order[0], len(hints))  # seed 991's own order
    ref = TR.TRef(dl, arrival, tp)
    st, n_counted, n_pairs = TR.host_target(seeds, hints, arrival, None, tp, H.HOST_M)
    assert (n_counted, n_pairs) == (ref.n_counted, ref.n_pairs)
    assert DR.same(st, ref.stats)
    assert int(st[1]["n_discordant"]) == 0 and int(st[1]["prefix_len"]) == len(hints)
