"""GPU: the replayable order sweep (nmz_replayable_order_sweep*, csrc/order.hip) against the numpy restatement over
the C oracle's delays (tests/order_ref.py). Everything is integer: every comparison is equality. No test depends on
a rate."""
import ctypes

import numpy as np
import pytest

import order_ref as R
from namazu_amd import _lib, replay
from namazu_amd.explorepolicy import Replayable
from oracle import oracle as O

pytestmark = pytest.mark.gpu

M = 10**8  # 100 ms
TIES_HINTS = ["same", "same", "twin", "twin", "other"]
TIES_ARRIVAL = [0, 3 * R.MS, 4 * R.MS, 4 * R.MS, 0]
TIES_CONS = [(0, 1, R.MS), (1, 0, R.MS), (2, 3, 1)]  # equal-hint pairs only: every seed has the same slacks


def policy(m=M):
    p = Replayable()
    p.MaxInterval = m
    return p


class Plan:
    """nmz_replayable_order_plan over one trace; sweeps into torch device buffers."""

    def __init__(self, ctx, hints, arrival, cons, m, max_seeds):
        self.L = _lib.load()
        ho, hb = O.to_csr(list(hints))
        arr = np.ascontiguousarray(arrival, np.int64)
        cs = Replayable.order_constraints(cons)
        self.h = ctypes.c_void_p()
        _lib.check(self.L.nmz_replayable_order_plan_create(ctx.handle, _lib.ptr(ho), _lib.ptr(hb), len(hints), m,
                                                           _lib.ptr(arr), _lib.ptr(cs), len(cs), max_seeds,
                                                           ctypes.byref(self.h)))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        _lib.check(self.L.nmz_replayable_order_plan_destroy(self.h))

    def enqueue(self, n, k, want_stats, lo=None, seeds=None, seed0=0, stream=None):
        import torch
        st = torch.zeros(max(n, 1) * 24, dtype=torch.uint8, device="cuda") if want_stats else None
        tk = torch.zeros(max(k, 1) * 24, dtype=torch.uint8, device="cuda")
        if stream is not None or not torch.cuda.current_stream().cuda_stream:
            # the buffers' zeroing ran on torch's current stream; the sweep runs on `stream`, or (torch's default
            # stream handle is NULL) on the context's own stream
            torch.cuda.current_stream().synchronize()
        s = ctypes.c_void_p((stream or torch.cuda.current_stream()).cuda_stream)
        p_st = ctypes.c_void_p(st.data_ptr()) if want_stats else None
        if seeds is None:
            _lib.check(self.L.nmz_replayable_order_sweep_decimal_dev(self.h, lo, n, k, p_st,
                                                                     ctypes.c_void_p(tk.data_ptr()), s))
            keep = ()
        else:
            so, sb = O.to_csr(seeds)
            keep = (torch.from_numpy(so.view(np.int32)).cuda(), torch.from_numpy(sb).cuda())
            _lib.check(self.L.nmz_replayable_order_sweep_dev(self.h, ctypes.c_void_p(keep[0].data_ptr()),
                                                             ctypes.c_void_p(keep[1].data_ptr()), n, seed0, k, p_st,
                                                             ctypes.c_void_p(tk.data_ptr()), s))
        return st, tk, keep

    @staticmethod
    def read(st, tk, n, k):
        import torch
        torch.cuda.synchronize()
        stats = np.frombuffer(st.cpu().numpy().tobytes(), _lib.ORDER_STATS_DTYPE)[:n] if st is not None else None
        return stats, np.frombuffer(tk.cpu().numpy().tobytes(), _lib.TOPK_DTYPE)[:k]

    def sweep(self, n, k, want_stats=True, **kw):
        st, tk, _keep = self.enqueue(n, k, want_stats, **kw)
        return self.read(st, tk, n, k)


def test_fixture_decimal_and_csr(ctx, golden):
    """F at 4,096 seeds through the decimal and the CSR host-pointer entry points (Replayable.OrderSweep)."""
    exp = R.fixture_stats(M)
    seeds, vals = R.decimal_seeds(0, 4096)
    want = R.topk(exp, vals, 64)
    p = policy()
    r = p.OrderSweep(R.F_HINTS, R.F_ARRIVAL, R.F_CONS, seed_lo=0, n_seeds=4096, k=64, ctx=ctx)
    assert R.same(r.stats, exp) and R.same(r.topk, want)
    r2 = p.OrderSweep(R.F_HINTS, R.F_ARRIVAL, R.F_CONS, seeds=seeds, k=64, ctx=ctx)
    assert R.same(r2.stats, exp) and R.same(r2.topk, want)  # seed = the CSR index = the decimal value here
    case = golden("order_sweep_kat.json")["cases"][str(M)]
    assert np.bincount(r.stats["n_satisfied"], minlength=6).tolist() == case["n_satisfied_histogram"]
    for got, w in zip(r.topk, case["top"]):
        assert (int(got["seed"]), int(got["n_fault"]), int(got["sum_delay_ns"]), int(got["first_fault"])) == \
            (w["seed"], w["n_satisfied"], w["min_slack_ns"], w["argmin_constraint"])
    # the top-k feeds the replay path unchanged
    best = replay.replayable_seeds(r2.topk, seeds)
    assert best[:2] == ["1029", "3880"] and replay.replay_env(best[0])[replay.REPLAY_SEED_ENV] == "1029"
    # without statistics: the same top-k, and no stats array
    r3 = p.OrderSweep(R.F_HINTS, R.F_ARRIVAL, R.F_CONS, seed_lo=0, n_seeds=4096, k=64, want_stats=False, ctx=ctx)
    assert r3.stats is None and R.same(r3.topk, want)


@pytest.mark.parametrize("lo", [0, 990, 2**64 - 616])  # 990: the range crosses 999 -> 1000; the last wraps past 2^64
@pytest.mark.parametrize("n", [1, 63, 65, 257, 4096])
def test_seed_ranges(ctx, lo, n):
    exp = R.fixture_stats(M, lo, n)
    seeds, vals = R.decimal_seeds(lo, n)
    with Plan(ctx, R.F_HINTS, R.F_ARRIVAL, R.F_CONS, M, n) as plan:
        for k in (1, 64, 256):  # n < k: sentinels past the seeds
            want = R.topk(exp, vals, k)
            st, tk = plan.sweep(n, k, lo=lo)
            assert R.same(st, exp) and R.same(tk, want)
            assert R.same(plan.sweep(n, k, want_stats=False, lo=lo)[1], want)  # d_stats == NULL
            if n < k:
                assert tuple(tk[n]) == R.SENTINEL and tuple(tk[-1]) == R.SENTINEL
        # the CSR of the same strings, seed = seed0 + index
        st, tk = plan.sweep(n, 64, seeds=seeds, seed0=5)
        assert R.same(st, exp) and R.same(tk, R.topk(exp, np.arange(n, dtype=np.uint64) + np.uint64(5), 64))
        st, _ = plan.sweep(n, 0, lo=lo)  # k == 0: statistics only
        assert R.same(st, exp)


@pytest.mark.parametrize("m", R.M_CASES)
def test_moduli(ctx, m):
    """m == 0, 1, a power of two, below 2^31, in [2^31, 2^32), above 2^32 and the largest: each kernel form."""
    lo, n = 990, 257
    exp = R.fixture_stats(m, lo, n)
    vals = R.decimal_seeds(lo, n)[1]
    with Plan(ctx, R.F_HINTS, R.F_ARRIVAL, R.F_CONS, m, n) as plan:
        st, tk = plan.sweep(n, 64, lo=lo)
    assert R.same(st, exp) and R.same(tk, R.topk(exp, vals, 64))


def test_kat_moduli_counts(ctx, golden):
    cases = golden("order_sweep_kat.json")["cases"]
    for m in (9 * 10**9, 2**20):
        r = policy(m).OrderSweep(R.F_HINTS, R.F_ARRIVAL, R.F_CONS, seed_lo=0, n_seeds=4096, k=64, ctx=ctx)
        assert R.same(r.stats, R.fixture_stats(m))
        hist = np.bincount(r.stats["n_satisfied"], minlength=6).tolist()
        if m == 2**20:  # nothing satisfied, one argmin: the top-k is ordered by min_slack alone
            assert hist == cases[str(m)]["n_satisfied_histogram"] and np.all(r.stats["argmin_constraint"] == 4)
            assert np.all(np.diff(r.topk["sum_delay_ns"]) <= 0)
            assert R.same(r.topk, R.topk(R.fixture_stats(m), np.arange(4096, dtype=np.uint64), 64))
        else:
            assert hist[5] == cases[str(m)]["n_all_satisfied"]


def test_csr_seeds_empty_seed_empty_hint_and_64_constraints(ctx):
    SEEDS = R.SEEDS
    hints, arrival, cons = R.wide_constraints()
    hints[7] = ""
    exp = R.stats(SEEDS, hints, arrival, cons, M)  # SEEDS starts with the empty seed, the reference's default
    r = policy().OrderSweep(hints, arrival, cons, seeds=SEEDS, k=8, ctx=ctx)
    assert R.same(r.stats, exp) and R.same(r.topk, R.topk(exp, np.arange(len(SEEDS), dtype=np.uint64), 8))
    assert np.all(r.stats["sat_mask"] >> np.uint64(63) == 1)
    r1 = policy().OrderSweep(hints, arrival, cons[:1], seeds=SEEDS, k=8, ctx=ctx)  # C == 1
    assert R.same(r1.stats, R.stats(SEEDS, hints, arrival, cons[:1], M))


@pytest.mark.parametrize("k", [64, 256])
def test_ties_take_the_lowest_seeds(ctx, k):
    """Only equal-hint pairs: every seed ties, over more than one block, so the top-k is the k lowest seeds."""
    lo, n = 2**64 - 616, 5000  # wraps: the lowest seed values are 0 .. 4383, after the wrap
    with Plan(ctx, TIES_HINTS, TIES_ARRIVAL, TIES_CONS, M, n) as plan:
        st, tk = plan.sweep(n, k, lo=lo)
        tk2 = plan.sweep(n, k, want_stats=False, lo=lo)[1]
    assert np.all(st["sat_mask"] == 0b001) and np.all(st["min_slack_ns"] == -4 * R.MS)
    assert np.all(st["argmin_constraint"] == 1) and np.all(st["n_satisfied"] == 1)
    assert tk["seed"].tolist() == list(range(k)) and np.all(tk["n_fault"] == 1)
    assert np.all(tk["sum_delay_ns"] == -4 * R.MS) and np.all(tk["first_fault"] == 1)
    assert tk.tobytes() == tk2.tobytes()


N_BIG = 2**16 + 3  # 33 blocks of 2,048 seeds, the last with 3


def test_fused_topk_over_many_blocks_and_merge(ctx):
    """2^16 + 3 seeds, k = 64: the per-block lists and their merge against the restatement; two half-range sweeps
    merged by nmz_topk_merge_dev equal the full range; nmz_replayable_order_host reproduces the top entries."""
    import torch
    lo, k = 123_456, 64
    exp = R.fixture_stats(M, lo, N_BIG)
    seeds, vals = R.decimal_seeds(lo, N_BIG)
    want = R.topk(exp, vals, k)
    L = _lib.load()
    with Plan(ctx, R.F_HINTS, R.F_ARRIVAL, R.F_CONS, M, N_BIG) as plan:
        st, tk = plan.sweep(N_BIG, k, lo=lo)
        assert R.same(st, exp) and R.same(tk, want)
        assert R.same(plan.sweep(N_BIG, k, want_stats=False, lo=lo)[1], want)
        half = N_BIG // 2
        # one real stream for torch's copies and the library's kernels (torch's default stream handle is NULL, which
        # the library reads as the context's own stream)
        with torch.cuda.stream(torch.cuda.Stream()):
            lists = torch.zeros(2 * k * 24, dtype=torch.uint8, device="cuda")
            for i, (a, cnt) in enumerate([(lo, half), (lo + half, N_BIG - half)]):
                _, part, _ = plan.enqueue(cnt, k, False, lo=a)
                lists[i * k * 24:(i + 1) * k * 24] = part
            scratch, out = torch.zeros_like(lists), torch.zeros(k * 24, dtype=torch.uint8, device="cuda")
            s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
            assert s.value
            _lib.check(L.nmz_topk_merge_dev(ctx.handle, ctypes.c_void_p(lists.data_ptr()), 2, k,
                                            ctypes.c_void_p(scratch.data_ptr()), ctypes.c_void_p(out.data_ptr()), s))
            assert R.same(Plan.read(None, out, 0, k)[1], want)
    top_seeds = [str(int(v)) for v in tk["seed"][:16]]
    hst, _ = R.host_order(top_seeds, R.F_HINTS, R.F_ARRIVAL, R.F_CONS, M)
    assert hst["n_satisfied"].tolist() == tk["n_fault"][:16].tolist()
    assert hst["min_slack_ns"].tolist() == tk["sum_delay_ns"][:16].tolist()
    assert hst["argmin_constraint"].tolist() == tk["first_fault"][:16].tolist()
    assert R.same(hst, exp[(tk["seed"][:16] - np.uint64(lo)).astype(np.int64)])


def test_plan_reuse_and_two_streams(ctx):
    import torch
    n, k = 4096, 64
    exp = R.fixture_stats(M)
    want = R.topk(exp, np.arange(n, dtype=np.uint64), k)
    with Plan(ctx, R.F_HINTS, R.F_ARRIVAL, R.F_CONS, M, n) as a, Plan(ctx, R.F_HINTS, R.F_ARRIVAL, R.F_CONS, M, n) as b:
        first = a.sweep(n, k, lo=0)
        a.sweep(100, 7, lo=555)  # another range in between leaves nothing behind
        second = a.sweep(n, k, lo=0)
        assert first[0].tobytes() == second[0].tobytes() and first[1].tobytes() == second[1].tobytes()
        assert R.same(first[0], exp) and R.same(first[1], want)
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        ra = a.enqueue(n, k, True, lo=0, stream=s1)
        rb = b.enqueue(n, k, True, lo=0, stream=s2)
        for st, tk, _ in (ra, rb):
            got = Plan.read(st, tk, n, k)
            assert R.same(got[0], exp) and R.same(got[1], want)


def test_sweep_argument_errors(ctx):
    with Plan(ctx, R.F_HINTS, R.F_ARRIVAL, R.F_CONS, M, 100) as plan:
        with pytest.raises(_lib.NmzInvalidArgument, match="more seeds than the plan"):
            plan.sweep(101, 1, lo=0)
        with pytest.raises(_lib.NmzInvalidArgument, match="k <= 256"):
            plan.sweep(100, 257, lo=0)
    with pytest.raises(_lib.NmzInvalidArgument, match="constraint 0: before == after"):
        Plan(ctx, R.F_HINTS, R.F_ARRIVAL, [(1, 1, 1)], M, 100)
    with pytest.raises(ValueError, match="either seeds or seed_lo"):
        policy().OrderSweep(R.F_HINTS, R.F_ARRIVAL, R.F_CONS, ctx=ctx)
    r = policy().OrderSweep(R.F_HINTS, R.F_ARRIVAL, R.F_CONS, seeds=[], k=2, ctx=ctx)  # no seeds: sentinels
    assert len(r.stats) == 0 and [tuple(e) for e in r.topk] == [R.SENTINEL] * 2
