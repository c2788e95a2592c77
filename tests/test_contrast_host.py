"""CPU: the order contrast's host pieces -- nmz_order_contrast_host (historystorage.order_pair) against the numpy
restatement (tests/contrast_ref.py) and against known answers written by plain Python loops
(tests/golden/order_contrast_kat.json), every NMZ_EINVAL with its message, run_positions on the ZooKeeper store,
replay.constraints_from_pairs, and the non-vacuity of the generated cases the GPU tests use."""
import numpy as np
import pytest

import contrast_ref as C
from namazu_amd import _lib, historystorage as hs, replay
from test_visualize import write_store, zk_store_traces

assert _lib.ORDER_PAIR_DTYPE == C.ORDER_PAIR_DTYPE  # the binding's record is the restatement's

# the generated cases of tests/test_contrast_gpu.py
GPU_CASES = [(1, 2), (1, 33), (2, 2), (2, 33), (63, 31), (63, 64), (64, 2), (64, 32), (64, 65), (65, 33), (65, 65),
             (127, 31), (127, 64), (129, 32), (129, 33), (129, 257), (130, 31), (257, 65), (257, 2), (2049, 3),
             (4096, 33)]


def pair_tuple(p):
    return (int(p["before"]), int(p["after"]), int(p["score"]), int(p["n_fail_with"]), int(p["n_pass_with"]),
            int(p["n_fail_against"]), int(p["n_pass_against"]))


@pytest.mark.parametrize("E,R", [(65, 33), (64, 2), (2, 33), (9, 5)])
def test_order_pair_equals_restatement_on_every_pair(E, R):
    pos, failed, F, P = C.case(E, R)
    n_fail = int(failed.sum())
    for b in range(E):
        for a in range(E):
            if a == b:
                continue
            got, nf, npass = hs.order_pair(pos, failed, b, a)
            assert pair_tuple(got) == C.one_pair(F, P, failed, b, a), (b, a)
            assert (nf, npass) == (n_fail, R - n_fail)


def test_equal_positions_count_for_neither_side():
    pos = np.array([[5, 5, 9], [5, 5, 1], [2, 8, 8], [7, 3, 3]], np.uint32)
    failed = np.array([1, 0, 1, 0], np.uint8)
    for b, a in [(0, 1), (1, 0)]:
        got, _, _ = hs.order_pair(pos, failed, b, a)
        # runs 0 and 1 hold both at position 5: neither direction; runs 2 and 3 order them
        assert pair_tuple(got) == (b, a, 2 if b == 0 else -2, 1 if b == 0 else 0, 0 if b == 0 else 1,
                                   0 if b == 0 else 1, 1 if b == 0 else 0)
    got, _, _ = hs.order_pair(pos, failed, 1, 2)
    assert pair_tuple(got) == (1, 2, 2, 1, 0, 0, 1)  # runs 2 and 3 hold events 1 and 2 at one position
    F, P = C.counts(pos, failed)
    assert F[0, 1] == 1 and F[1, 0] == 0 and P[0, 1] == 0 and P[1, 0] == 1


def test_every_einval_has_its_message():
    pos = np.arange(12, dtype=np.uint32).reshape(3, 4)
    ok = np.array([1, 0, 0], np.uint8)

    def bad(match, p=pos, f=ok, b=0, a=1):
        with pytest.raises(_lib.NmzInvalidArgument, match=match):
            hs.order_pair(p, f, b, a)

    bad("no failing run", f=np.zeros(3, np.uint8))
    bad("no passing run", f=np.ones(3, np.uint8))
    bad(r"failed\[1\] must be 0 or 1", f=np.array([1, 2, 0], np.uint8))
    bad(r"n_events must be in \[1, 4096\]", p=np.zeros((3, 0), np.uint32))
    bad(r"n_events must be in \[1, 4096\]", p=np.zeros((3, 4097), np.uint32))
    bad(r"n_runs must be in \[1, 65535\]", p=np.zeros((65536, 2), np.uint32),
        f=np.r_[1, np.zeros(65535)].astype(np.uint8))
    bad("before == after", b=2, a=2)
    bad("event index out of range", b=0, a=4)
    with pytest.raises(ValueError, match="labels for"):
        hs.order_pair(pos, ok[:2], 0, 1)
    # the device forms check their arguments before they look at the context: no device is needed to be refused
    L = _lib.load()
    pairs = np.zeros(300, _lib.ORDER_PAIR_DTYPE)

    def refused(msg, *args):
        assert L.nmz_order_contrast(None, *args) == _lib.NMZ_EINVAL
        assert msg in _lib.last_error(), _lib.last_error()

    refused("top-k supports k <= 256", _lib.ptr(pos), _lib.ptr(ok), 3, 4, 257, None, _lib.ptr(pairs), None)
    refused("n_events must be in [1, 4096]", _lib.ptr(pos), _lib.ptr(ok), 3, 0, 8, None, _lib.ptr(pairs), None)
    refused("n_events must be in [1, 4096]", _lib.ptr(pos), _lib.ptr(ok), 3, 4097, 8, None, _lib.ptr(pairs), None)
    refused("n_runs must be in [1, 65535]", _lib.ptr(pos), _lib.ptr(ok), 65536, 4, 8, None, _lib.ptr(pairs), None)
    refused("no failing run", _lib.ptr(pos), _lib.ptr(np.zeros(3, np.uint8)), 3, 4, 8, None, _lib.ptr(pairs), None)
    refused("no passing run", _lib.ptr(pos), _lib.ptr(np.ones(3, np.uint8)), 3, 4, 8, None, _lib.ptr(pairs), None)
    refused("failed[2] must be 0 or 1", _lib.ptr(pos), _lib.ptr(np.array([1, 0, 2], np.uint8)), 3, 4, 8, None,
            _lib.ptr(pairs), None)
    refused("ctx is NULL", _lib.ptr(pos), _lib.ptr(ok), 3, 4, 8, None, _lib.ptr(pairs), None)
    assert L.nmz_order_contrast_dev(None, None, None, 3, 4, 8, None, None, None, None) == _lib.NMZ_EINVAL
    assert "ctx is NULL" in _lib.last_error()


def test_known_answers(golden):
    kat = golden("order_contrast_kat.json")["cases"]
    assert len(kat) >= 4
    saw_absent = saw_equal = False
    for c in kat:
        pos = np.array(c["pos"], np.uint32)
        failed = np.array(c["failed"], np.uint8)
        E, R = c["n_events"], c["n_runs"]
        assert pos.shape == (R, E)
        saw_absent |= bool((pos == C.NONE).any())
        saw_equal |= any(len(set(row[row != C.NONE].tolist())) < int((row != C.NONE).sum()) for row in pos)
        # the restatement against the plain loops
        F, P = C.counts(pos, failed)
        assert F.tolist() == c["F"] and P.tolist() == c["P"]
        assert C.scores(F, P, failed).tolist() == c["score"]
        exp, n_positive = C.ranked(F, P, failed, E * E)
        assert n_positive == len(c["ranked"])
        assert [list(pair_tuple(p)) for p in exp[:n_positive]] == c["ranked"]
        # the host entry point against the plain loops
        for b in range(E):
            for a in range(E):
                if a == b:
                    continue
                got, nf, npass = hs.order_pair(pos, failed, b, a)
                assert pair_tuple(got) == (b, a, c["score"][b][a], c["F"][b][a], c["P"][b][a], c["F"][a][b],
                                           c["P"][a][b])
                assert (nf, npass) == (c["n_fail"], c["n_pass"])
    assert saw_absent and saw_equal


def test_run_positions_on_the_zk_store(golden, tmp_path):
    traces = zk_store_traces(golden)
    write_store(str(tmp_path), traces)
    st = hs.LoadStorage(str(tmp_path))
    runs = st.traces()
    sym = runs[0].symbols  # trace 0's events are the universe, arrival = index
    arr = np.arange(len(sym), dtype=np.int64)
    pos = hs.run_positions(sym, arr, runs)
    assert pos.shape == (6, 48) and pos.dtype == np.uint32
    assert np.array_equal(pos[0], np.arange(48, dtype=np.uint32))
    assert np.array_equal(pos[5], pos[0])  # the Event-equal replay
    assert np.array_equal(pos[4], pos[0])  # the re-recorded run holds the same events
    for r in range(6):
        assert np.array_equal(pos[r], hs.match_target(sym, arr, runs[r].symbols))
    # symbol arrays pass as well as SingleTraces
    assert np.array_equal(hs.run_positions(sym, arr, [t.symbols for t in runs]), pos)


def test_constraints_from_pairs():
    S = (C.NONE, C.NONE, C.INT64_MIN, 0, 0, 0, 0)
    pairs = np.array([(7, 3, 90, 9, 0, 0, 9), (7, 4, 80, 8, 0, 0, 8), (3, 7, 70, 7, 0, 0, 7), (7, 5, 60, 6, 0, 0, 6),
                      (1, 2, 50, 5, 0, 0, 5), (2, 1, 40, 4, 0, 0, 4), (5, 6, 30, 3, 0, 0, 3), S, (8, 9, 1, 1, 0, 0, 1)],
                     _lib.ORDER_PAIR_DTYPE)
    m = 1_000_000
    # order kept, the reverse pairs (3, 7) and (2, 1) dropped, the sentinel stops the list
    assert replay.constraints_from_pairs(pairs, m) == [(7, 3, m), (7, 4, m), (7, 5, m), (1, 2, m), (5, 6, m)]
    assert replay.constraints_from_pairs(pairs, m, max_constraints=2) == [(7, 3, m), (7, 4, m)]
    # at most two constraints may name event 7; (5, 6) still fits (5 was named by no kept constraint)
    assert replay.constraints_from_pairs(pairs, m, per_event=2) == [(7, 3, m), (7, 4, m), (1, 2, m), (5, 6, m)]
    assert replay.constraints_from_pairs(pairs, m, per_event=1) == [(7, 3, m), (1, 2, m), (5, 6, m)]
    assert replay.constraints_from_pairs(pairs[7:], m) == []
    assert replay.constraints_from_pairs(pairs[:0], m) == []
    with pytest.raises(ValueError):
        replay.constraints_from_pairs(pairs, m, per_event=0)


@pytest.mark.parametrize("E,R", [c for c in GPU_CASES if c[0] >= 2])
def test_generated_cases_are_not_vacuous(E, R):
    """From the restatement alone: enough absences, enough positive pairs, and for E >= 64 a tie at the k = 64 cut."""
    pos, failed, F, P = C.case(E, R)
    assert 0 < failed.sum() < R
    if E >= 9:
        assert (pos == C.NONE).mean() >= 0.10
    sc = C.scores(F, P, failed)
    off = ~np.eye(E, dtype=bool)
    if R >= 31 or E >= 64:
        assert (sc[off] > 0).mean() >= 0.15
    if E >= 64:
        flat = sc[off]
        top = np.sort(np.partition(flat, len(flat) - 65)[-65:])[::-1]
        assert top[63] == top[64] and top[63] > 0


def test_the_planted_pair_leads():
    for E, R in [(65, 33), (130, 31), (257, 65)]:
        pos, failed, F, P = C.case(E, R)
        exp, _ = C.ranked(F, P, failed, 1)
        assert (int(exp[0]["before"]), int(exp[0]["after"])) == (7, 3)
