"""CPU: nmz_match_run_host (plain loops, no device) against historystorage.match_target (numpy) on the whole grid of
tests/match_cases.py and on the hand cases of test_target_host.py::test_match_target; every NMZ_EINVAL of the host
forms with its message, raised before any context is needed; and the grid itself is not vacuous."""
import ctypes

import numpy as np
import pytest

import match_cases as M
from namazu_amd import _lib, historystorage as hs

NONE = _lib.NMZ_NONE


@pytest.mark.parametrize("E,U", M.CASES)
def test_host_equals_match_target_on_the_grid(E, U):
    sym, arrival, runs, exp = M.case(E, U)
    for r, run in enumerate(runs):
        got = hs.match_run_host(sym, arrival, run)
        assert got.dtype == np.uint32 and np.array_equal(got, exp[r]), f"run {r} of length {len(run)}"


def test_host_hand_cases():
    assert hs.match_run_host([5, 7, 5, 9, 5], [10, 0, 3, 1, 3], [5, 5, 7, 8, 5, 5]).tolist() == [4, 2, 0, NONE, 1]
    # more events than recorded occurrences: the latest arrivals stay unmatched
    assert hs.match_run_host([1, 1, 1], [30, 10, 20], [1, 2, 1]).tolist() == [NONE, 0, 2]
    assert hs.match_run_host([1, 2], [0, 0], []).tolist() == [NONE, NONE]
    with pytest.raises(ValueError, match="arrival times"):
        hs.match_run_host([1, 2], [0], [1])
    # distinct symbols: the inverse of the recorded order, whatever the arrivals
    rng = np.random.default_rng(4)
    sym = rng.permutation(2**20)[:50].astype(np.uint64)
    rec = sym[rng.permutation(50)]
    tp = hs.match_run_host(sym, rng.integers(0, 5, 50), rec)
    assert np.array_equal(rec[tp], sym)
    # negative arrivals order as signed numbers
    assert hs.match_run_host([3, 3], [5, -5], [3]).tolist() == [NONE, 0]


@pytest.mark.parametrize("E,U", M.CASES)
def test_the_grid_is_not_vacuous(E, U):
    """Conditions on the generator, from numpy alone (over the base lengths): every case has at least 15 % NMZ_NONE
    cells, at least 85 % matched cells among the runs with L >= E, at least one (run, symbol) pair with more
    occurrences than the universe holds, and, from 64 events on, arrival ties."""
    sym, arrival, runs, exp = M.case(E, U)
    nb = len(M.BASE_LENGTHS)
    assert [len(r) for r in runs] == M.LENGTHS
    assert len(np.unique(sym)) == U
    none = (exp[:nb] == NONE).mean()
    full = [i for i, L in enumerate(M.BASE_LENGTHS) if L >= E]
    matched = (exp[full] != NONE).mean()
    print(f"E={E} U={U}: none {none:.3f} matched {matched:.3f} over-full {M.over_full_pairs(sym, runs[:nb])}")
    assert none >= 0.15
    assert matched >= 0.85
    assert M.over_full_pairs(sym, runs[:nb]) >= 1
    if E >= 64:
        assert len(np.unique(arrival)) < E
    if U >= 4:  # the awkward values are there
        vals = set(sym.tolist())
        assert 0 in vals and 2**64 - 1 in vals
        low = [v & 0xFFFFFFFF for v in vals]
        assert len(set(low)) < len(low)


# ---- the limits, each NMZ_EINVAL with its message, before any context -------------------------------------------
def _u64(*v):
    return np.array(v, np.uint64)


def _host(sym, arr, E, run, n, pos):
    return _lib.load().nmz_match_run_host(_lib.ptr(sym), _lib.ptr(arr), E, _lib.ptr(run), n, _lib.ptr(pos))


def _runs(sym, arr, E, off, rs, R, pos, ctx=None):
    return _lib.load().nmz_match_runs(ctx, _lib.ptr(sym), _lib.ptr(arr), E, _lib.ptr(off), _lib.ptr(rs), R,
                                      _lib.ptr(pos))


def _einval(rc, text):
    assert rc == _lib.NMZ_EINVAL
    assert text in _lib.last_error(), _lib.last_error()


def test_host_form_limits():
    sym, arr, run = _u64(1, 2), np.zeros(2, np.int64), _u64(1)
    pos = np.zeros(2, np.uint32)
    _einval(_host(sym, arr, 0, run, 1, pos), "n_events must be in [1, 4096]")
    _einval(_host(sym, arr, 4097, run, 1, pos), "n_events must be in [1, 4096]")
    _einval(_host(None, arr, 2, run, 1, pos), "sym or arrival_ns is NULL")
    _einval(_host(sym, None, 2, run, 1, pos), "sym or arrival_ns is NULL")
    _einval(_host(sym, arr, 2, run, 2**32 - 1, pos), "at most 2^32 - 2")
    _einval(_host(sym, arr, 2, None, 1, pos), "run_sym is NULL")
    _einval(_host(sym, arr, 2, run, 1, None), "pos is NULL")
    assert _host(sym, arr, 2, None, 0, pos) == _lib.NMZ_OK and pos.tolist() == [NONE, NONE]


def test_match_runs_limits_need_no_context():
    sym, arr = _u64(1, 2), np.zeros(2, np.int64)
    off, rs = _u64(0, 1, 2), _u64(1, 2)
    pos = np.zeros((2, 2), np.uint32)
    _einval(_runs(sym, arr, 0, off, rs, 2, pos), "n_events must be in [1, 4096]")
    _einval(_runs(sym, arr, 4097, off, rs, 2, pos), "n_events must be in [1, 4096]")
    _einval(_runs(None, arr, 2, off, rs, 2, pos), "sym or arrival_ns is NULL")
    _einval(_runs(sym, arr, 2, off, rs, 2**63, pos), "n_runs * n_events does not fit the output")
    _einval(_runs(sym, arr, 2, None, rs, 2, pos), "run_off is NULL")
    _einval(_runs(sym, arr, 2, _u64(1, 1, 2), rs, 2, pos), "run_off[0] must be 0")
    _einval(_runs(sym, arr, 2, _u64(0, 2, 1), rs, 2, pos), "run_off must be non-decreasing (run 1)")
    _einval(_runs(sym, arr, 2, _u64(0, 1, 2**32), rs, 2, pos), "run 1 has 4294967295 elements: at most 2^32 - 2")
    _einval(_runs(sym, arr, 2, off, None, 2, pos), "run_sym is NULL")
    _einval(_runs(sym, arr, 2, off, rs, 2, None), "pos is NULL")
    # everything in order: only the context is missing
    _einval(_runs(sym, arr, 2, off, rs, 2, pos), "ctx is NULL")
    # no runs: legal, nothing is written, and no device is needed
    pos[:] = 7
    assert _runs(sym, arr, 2, None, None, 0, pos) == _lib.NMZ_OK and (pos == 7).all()


def test_plan_and_dev_form_null_arguments():
    L = _lib.load()
    out = ctypes.c_void_p()
    _einval(L.nmz_match_plan_create(None, None, None, 1, ctypes.byref(out)), "NULL argument")
    assert L.nmz_match_plan_destroy(None) == _lib.NMZ_OK
    _einval(L.nmz_match_plan_info(None, None, None), "plan is NULL")
    _einval(L.nmz_match_runs_dev(None, None, None, 0, None, None), "plan is NULL")


def test_order_contrast_runs_limits_need_no_context():
    """nmz_order_contrast's limits and label checks with the same messages, and the matching's, before any device
    work."""
    L = _lib.load()
    sym, arr = _u64(1, 2), np.zeros(2, np.int64)
    off, rs = _u64(0, 1, 2), _u64(1, 2)

    def call(E=2, off=off, rs=rs, failed=np.array([1, 0], np.uint8), R=2, k=4, sym=sym):
        pairs = np.zeros(max(k, 1), _lib.ORDER_PAIR_DTYPE)
        return L.nmz_order_contrast_runs(None, _lib.ptr(sym), _lib.ptr(arr), E, _lib.ptr(off), _lib.ptr(rs),
                                         _lib.ptr(failed), R, min(k, 2**32 - 1), None, _lib.ptr(pairs), None)

    _einval(call(E=0), "n_events must be in [1, 4096]")
    _einval(call(E=4097), "n_events must be in [1, 4096]")
    _einval(call(R=0), "n_runs must be in [1, 65535]")
    _einval(call(R=65536), "n_runs must be in [1, 65535]")
    _einval(call(k=257), "top-k supports k <= 256")
    _einval(call(sym=None), "sym or arrival_ns is NULL")
    _einval(call(off=_u64(1, 1, 2)), "run_off[0] must be 0")
    _einval(call(off=_u64(0, 2, 1)), "run_off must be non-decreasing (run 1)")
    _einval(call(off=_u64(0, 1, 2**32)), "at most 2^32 - 2")
    _einval(call(rs=None), "run_sym is NULL")
    _einval(call(failed=None), "failed is NULL")
    _einval(call(failed=np.array([1, 2], np.uint8)), "failed[1] must be 0 or 1")
    _einval(call(failed=np.array([0, 0], np.uint8)), "no failing run: nothing to contrast")
    _einval(call(failed=np.array([1, 1], np.uint8)), "no passing run: nothing to contrast")
    _einval(call(), "ctx is NULL")


def test_python_argument_checks():
    with pytest.raises(ValueError, match="arrival times"):
        hs.match_runs([1, 2], [0], [[1]])
    with pytest.raises(ValueError, match="labels for"):
        hs.order_contrast_runs([1, 2], [0, 0], [[1], [2]], [1])
    with pytest.raises(_lib.NmzInvalidArgument, match="n_events must be in"):
        hs.match_run_host([], [], [1])
