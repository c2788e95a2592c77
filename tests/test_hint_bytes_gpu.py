"""GPU parity on long and non-ASCII replay hints (tests/hint_cases.py): every K1 plan form, the online decisions,
the sweeps that build their tables on the host, and seed bytes at unaligned device addresses, against the plain
reference of the delays (hint_cases.reference_delays) and the C oracle's statistics records, which
tests/test_hint_bytes.py shows equal to the reference's on these very inputs. Bit-exact comparison everywhere."""
import ctypes
import functools

import numpy as np
import pytest

import delivery_ref as DR
import hint_cases as H
import order_ref as OR
import target_ref as TR
from namazu_amd import _lib
from namazu_amd.explorepolicy import Replayable, to_csr
from oracle import oracle as O
from test_sweeps_gpu import k1  # noqa: F401

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def expected(name, m):
    """(oracle stats[S], reference delays[S, E]) of a family under modulus m; computed once, shared, read-only."""
    hints, seeds = H.FAMILIES[name](), H.family_seeds(name)
    so, sb = O.to_csr(seeds)
    ho, hb = O.to_csr(hints)
    st, _ = O.replayable_sweep(so, sb, ho, hb, m)
    st.setflags(write=False)
    dl = H.reference_delays(seeds, hints, m)
    dl.setflags(write=False)
    return st, dl


def plan_kernel(ctx, hints, m, max_seeds=512):
    """nmz_replayable_plan_kernel of a plan over the hints, under the environment of the moment: 2 the wavelet
    trees, 1 the order queries, 0 the per-decision sweeps."""
    L = _lib.load()
    ho, hb = to_csr(hints)
    plan = ctypes.c_void_p()
    _lib.check(L.nmz_replayable_plan_create(ctx.handle, _lib.ptr(ho), _lib.ptr(hb), len(hints), m, max_seeds,
                                            ctypes.byref(plan)))
    try:
        return L.nmz_replayable_plan_kernel(plan)
    finally:
        L.nmz_replayable_plan_destroy(plan)


def first_wrong_event(ctx, seeds, hints, m):
    """For a failure message: the statistics cannot name the event whose delay was wrong, so sweep prefixes of the
    trace (a prefix keeps every hint's offset, hence its alignment) and bisect for the shortest one whose stats
    differ from the oracle's; its last event is the first one the plan got wrong."""
    so, sb = O.to_csr(seeds)
    p = Replayable()
    p.MaxInterval = m

    def wrong(n):
        ho, hb = O.to_csr(hints[:n])
        return not np.array_equal(p.Sweep(seeds, hints[:n], ctx=ctx).stats, O.replayable_sweep(so, sb, ho, hb, m)[0])

    lo, hi = 0, len(hints)  # stats of the empty prefix are right, those of the whole trace are not
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if wrong(mid) else (mid, hi)
    off = H.hint_offsets(hints)
    return (f"; first event with a wrong delay (by prefixes of the trace): event {hi - 1}, hint length "
            f"{len(hints[hi - 1])}, hint_off[e] & 3 = {int(off[hi - 1]) & 3}")


def check_sweep(ctx, name, m, n_dump=None):
    hints, seeds = H.FAMILIES[name](), H.family_seeds(name)
    n_dump = len(seeds) if n_dump is None else n_dump
    st, dl = expected(name, m)
    p = Replayable()
    p.MaxInterval = m
    r = p.Sweep(seeds, hints, n_dump=n_dump, k=10, ctx=ctx)
    assert np.array_equal(r.delays, dl[:n_dump]), H.first_difference(r.delays, dl[:n_dump], hints)
    if not np.array_equal(r.stats, st):
        raise AssertionError(H.stats_difference(r.stats, st, hints) + first_wrong_event(ctx, seeds, hints, m))
    assert np.array_equal(r.topk, O.topk_from_stats(st, 0, 10))


# ---------------------------------------------------------------- every K1 plan form on the joints
@pytest.mark.parametrize("m", [7, 10**8, 2**30 + 5, 2**31 + 3, 2**32 + 7])
@pytest.mark.parametrize("name", ["joints", "joints_tail2", "joints_tail3", "joints_tail0"])
def test_joints(ctx, k1, name, m):  # noqa: F811
    """Hints of the fused plan reader's lengths (0 .. 1,000 bytes: up to 63 rounds of 16) at every start alignment,
    bytes of every value, totals of every residue mod 4 (the last word clamp on a partial dword): stats, every delay
    and the top-k. The default form must have run the wavelet-tree kernel, or the fused reader was not tested."""
    if k1 == "wt" and m < 2**32:
        assert plan_kernel(ctx, H.FAMILIES[name](), m) == 2
    check_sweep(ctx, name, m)


# ---------------------------------------------------------------- the long hint
@pytest.mark.parametrize("m", [10**8, 2**32 + 7])
@pytest.mark.parametrize("extra", [0, 1])
@pytest.mark.parametrize("E", [5, 300])
@pytest.mark.parametrize("k1", ["wt", "wt_sep", "oq", "pd"], indirect=True)
def test_one_long_hint(ctx, k1, E, extra, m):  # noqa: F811
    """One hint of 4 E + 4096 (+ 1) bytes among short ones: plan_create's counting sort with its largest position
    vector, and one byte further its comparison sort; the plan kernels read the long hint in hundreds of rounds.
    (The rank-block widths do not change how hints are read: wt stands for them.) The default form must have run
    the wavelet-tree kernel, or the fused reader did not read the long hint."""
    if k1 == "wt" and m < 2**32:
        assert plan_kernel(ctx, H.one_long(E, extra), m) == 2
    check_sweep(ctx, f"one_long_{E}_{extra}", m)


# ---------------------------------------------------------------- class structure
# nmz_replayable_plan_kernel as observed on an MI355X, per form: 700 classes of 1 and the 4,097-event class (two
# sub-segments) run the wavelet trees; 90 classes of 9 exceed LDS with 64-rank blocks (~177 KB of row image) and
# fit with 32-rank blocks (~141 KB), so the plan narrows the blocks and keeps the wavelet trees
PLAN_KERNEL = {("many_classes", "wt"): 2, ("many_classes", "wt_sep"): 2, ("many_classes", "oq"): 1,
               ("mid_classes", "wt"): 2, ("mid_classes", "wt_sep"): 2, ("mid_classes", "oq"): 1,
               ("long_class", "wt"): 2, ("long_class", "wt_sep"): 2, ("long_class", "oq"): 1}


@pytest.mark.parametrize("m", [7, 10**8])
@pytest.mark.parametrize("name", ["many_classes", "mid_classes", "long_class"])
@pytest.mark.parametrize("k1", ["wt", "wt_sep", "oq"], indirect=True)
def test_class_structure(ctx, k1, name, m):  # noqa: F811
    """700 classes of 1 (hints of 0..699 bytes), 90 classes just above WT_BRUTE, and one class of 4,097 64-byte
    hints (two wavelet-tree sub-segments, four full rounds); the plan kernel each form takes is the recorded one."""
    assert plan_kernel(ctx, H.FAMILIES[name](), m) == PLAN_KERNEL[name, k1]
    check_sweep(ctx, name, m, n_dump=2 if name == "long_class" else None)


# ---------------------------------------------------------------- online decisions
@pytest.mark.parametrize("m", [10**8, 2**63 - 1, 0])
@pytest.mark.parametrize("name", ["joints", "one_long_5_1"])
def test_decide_device(ctx, name, m):
    """nmz_replayable_decide (k_replayable_dump's byte loop) for six seeds, the empty one and 0xff bytes among them."""
    L = _lib.load()
    hints = H.FAMILIES[name]()
    seeds = [H.seeds()[i] for i in H.DECIDE_SEEDS]
    assert b"" in seeds and b"\xff" * 7 in seeds
    ho, hb = to_csr(hints)
    ref = H.reference_delays(seeds, hints, m)
    got = np.full_like(ref, -1)
    for i, s in enumerate(seeds):
        sb = np.frombuffer(s, np.uint8) if s else np.zeros(1, np.uint8)
        _lib.check(L.nmz_replayable_decide(ctx.handle, _lib.ptr(sb), len(s), _lib.ptr(ho), _lib.ptr(hb), len(hints),
                                           m, _lib.ptr(got[i])))
    assert np.array_equal(got, ref), H.first_difference(got, ref, hints)


# ---------------------------------------------------------------- the sweeps that build their tables on the host
def seed_kw(kind):
    if kind == "csr":
        return dict(seeds=H.host_sweep_seeds()), np.arange(H.HOST_N_SEEDS, dtype=np.uint64)
    return (dict(seed_lo=H.HOST_SEED_LO, n_seeds=H.HOST_N_SEEDS),
            np.arange(H.HOST_SEED_LO, H.HOST_SEED_LO + H.HOST_N_SEEDS, dtype=np.uint64))


@functools.lru_cache(maxsize=None)
def host_case():
    """joints() under 10^8 ns for the decimal seeds 990 .. 1289: (hints, reference delays, arrival, sym)."""
    hints = H.joints()
    _, arrival, sym, _ = DR.case_inputs(len(hints), H.HOST_M)
    return hints, H.reference_delays(H.host_sweep_seeds(), hints, H.HOST_M), arrival, sym


def policy():
    p = Replayable()
    p.MaxInterval = H.HOST_M
    return p


@pytest.mark.parametrize("kind", ["csr", "decimal"])
def test_order_sweep(ctx, kind):
    hints, dl, _, _ = host_case()
    cons, arrival = H.order_constraints(hints), np.zeros(len(hints), np.int64)
    exp = OR.stats_from_slack(OR.slacks(dl, arrival, cons))
    kw, vals = seed_kw(kind)
    r = policy().OrderSweep(hints, arrival, cons, k=8, ctx=ctx, **kw)
    assert OR.same(r.stats, exp)
    assert OR.same(r.topk, OR.topk(exp, vals, 8))


@pytest.mark.parametrize("kind", ["csr", "decimal"])
def test_delivery_orders(ctx, kind):
    hints, dl, arrival, sym = host_case()
    ref = DR.Ref(dl, arrival, sym)
    r = policy().DeliveryOrders(hints, arrival, sym, ctx=ctx, **seed_kw(kind)[0])
    assert DR.same(r.stats, ref.stats)
    assert np.array_equal(r.first_equal, ref.first_equal()) and np.array_equal(r.class_rep, ref.class_rep())
    assert r.n_classes == len(set(ref.first_equal().tolist()))


@pytest.mark.parametrize("kind", ["csr", "decimal"])
def test_nearest_orders(ctx, kind):
    hints, dl, arrival, sym = host_case()
    tp = TR.target_of_order(DR.Ref(dl[1:2], arrival, sym).order[0], len(hints))  # seed 991's own order
    ref = TR.TRef(dl, arrival, tp)
    kw, vals = seed_kw(kind)
    r = policy().NearestOrders(hints, arrival, target_pos=tp, k=8, ctx=ctx, **kw)
    assert (r.n_counted, r.n_pairs) == (ref.n_counted, ref.n_pairs)
    assert DR.same(r.stats, ref.stats)
    assert np.array_equal(r.topk.astype(TR.TOPK_DTYPE), TR.topk(ref.stats, ref.n_pairs, vals, 8, "pairs"))
    assert int(r.stats[1]["n_discordant"]) == 0


# ---------------------------------------------------------------- unaligned seed bytes on the device forms
@pytest.mark.parametrize("kind", ["decimal_strings", "random_bytes"])
def test_unaligned_seed_bytes(ctx, kind):
    """k_seed_prefix takes its staging offset from the address of the seed bytes: the same CSR at device addresses
    1, 2 and 3 past a dword boundary gives the aligned call's stats, which are the oracle's. 5,000 short decimal
    seeds (blocks staged in LDS) and 3,000 seeds of 0..60 random bytes (blocks beyond the staging's 16 KB)."""
    import torch
    L = _lib.load()
    if kind == "decimal_strings":
        seeds = [str(i * 7919).encode() for i in range(5000)]
    else:
        rng = np.random.default_rng(60)
        seeds = [rng.integers(0, 256, int(rng.integers(0, 61)), dtype=np.uint8).tobytes() for _ in range(3000)]
    hints, m, S = H.joints(), 10**8, len(seeds)
    so, sb = to_csr(seeds)
    ho, hb = to_csr(hints)
    exp, _ = O.replayable_sweep(*O.to_csr(seeds), ho, hb, m)
    plan = ctypes.c_void_p()
    _lib.check(L.nmz_replayable_plan_create(ctx.handle, _lib.ptr(ho), _lib.ptr(hb), len(hints), m, S,
                                            ctypes.byref(plan)))
    try:
        d_so = torch.from_numpy(so.view(np.int32)).cuda()
        buf = torch.zeros(len(sb) + 16, dtype=torch.uint8, device="cuda")
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        for o in (0, 1, 2, 3):
            start = (-buf.data_ptr()) % 4 + o
            assert (buf.data_ptr() + start) % 4 == o and start + len(sb) <= buf.numel()
            buf.zero_()
            buf[start:start + len(sb)] = torch.from_numpy(sb).cuda()
            d_st = torch.zeros(S * 32, dtype=torch.uint8, device="cuda")
            _lib.check(L.nmz_replayable_sweep_dev(plan, ctypes.c_void_p(d_so.data_ptr()),
                                                  ctypes.c_void_p(buf.data_ptr() + start), S,
                                                  ctypes.c_void_p(d_st.data_ptr()), stream))
            torch.cuda.synchronize()
            got = np.frombuffer(d_st.cpu().numpy().tobytes(), dtype=_lib.SCHED_STATS_DTYPE)
            assert np.array_equal(got, exp), (o, H.stats_difference(got, exp, hints))
    finally:
        L.nmz_replayable_plan_destroy(plan)
