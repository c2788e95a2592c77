"""GPU: the delivery sweep and its class builder (nmz_replayable_delivery_*, nmz_delivery_classes_dev,
nmz_sig_classes_dev; csrc/delivery.hip) against nmz_replayable_delivery_host, the numpy restatement over the C
oracle's delays (tests/delivery_ref.py), the project's own trace signatures and classes (nmz_trace_signatures,
nmz_unique_traces) and the reference's literal loops (oracle.unique_curve_*). Everything is integer: every
comparison is equality. No test depends on a rate."""
import ctypes
import functools

import numpy as np
import pytest

import delivery_ref as R
from namazu_amd import _lib
from namazu_amd.explorepolicy import Replayable
from oracle import oracle as O

pytestmark = pytest.mark.gpu
MS = R.MS


def _vp(t):
    return ctypes.c_void_p(t.data_ptr())


class Plan:
    """nmz_replayable_delivery_plan over one trace; sweeps and classes into torch device buffers."""

    def __init__(self, ctx, hints, arrival, sym, entity, m, max_seeds):
        self.L, self.ctx = _lib.load(), ctx
        ho, hb = O.to_csr(list(hints))
        arr = np.ascontiguousarray(arrival, np.int64)
        sy = np.ascontiguousarray(sym, np.uint64)
        en = None if entity is None else np.ascontiguousarray(entity, np.uint32)
        self.h = ctypes.c_void_p()
        _lib.check(self.L.nmz_replayable_delivery_plan_create(ctx.handle, _lib.ptr(ho), _lib.ptr(hb), len(hints), m,
                                                              _lib.ptr(arr), _lib.ptr(sy), _lib.ptr(en), max_seeds,
                                                              ctypes.byref(self.h)))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        _lib.check(self.L.nmz_replayable_delivery_plan_destroy(self.h))

    def enqueue(self, n, lo=None, seeds=None, stream=None):
        import torch
        st = torch.zeros(max(n, 1) * 32, dtype=torch.uint8, device="cuda")
        if stream is not None or not torch.cuda.current_stream().cuda_stream:
            # the buffer's zeroing ran on torch's current stream; the sweep runs on `stream`, or (torch's default
            # stream handle is NULL) on the context's own stream
            torch.cuda.current_stream().synchronize()
        s = ctypes.c_void_p((stream or torch.cuda.current_stream()).cuda_stream)
        if seeds is None:
            _lib.check(self.L.nmz_replayable_delivery_sweep_decimal_dev(self.h, lo, n, _vp(st), s))
            keep = ()
        else:
            so, sb = O.to_csr(seeds)
            keep = (torch.from_numpy(so.view(np.int32)).cuda(), torch.from_numpy(sb).cuda())
            torch.cuda.current_stream().synchronize()
            _lib.check(self.L.nmz_replayable_delivery_sweep_dev(self.h, _vp(keep[0]), _vp(keep[1]), n, _vp(st), s))
        return st, s, keep

    def classes(self, st, n, s):
        import torch
        fe = torch.zeros(max(n, 1), dtype=torch.int32, device="cuda")
        rep = torch.zeros(max(n, 1), dtype=torch.int32, device="cuda")
        nc = torch.full((1,), 77, dtype=torch.int32, device="cuda")
        torch.cuda.current_stream().synchronize()
        _lib.check(self.L.nmz_delivery_classes_dev(self.ctx.handle, _vp(st), n, _vp(fe), _vp(rep), _vp(nc), s))
        torch.cuda.synchronize()
        return (fe.cpu().numpy().view(np.uint32)[:n], rep.cpu().numpy().view(np.uint32)[:n],
                int(nc.cpu().numpy().view(np.uint32)[0]))

    @staticmethod
    def read(st, n):
        import torch
        torch.cuda.synchronize()
        return np.frombuffer(st.cpu().numpy().tobytes(), _lib.DELIVERY_STATS_DTYPE)[:n]

    def sweep(self, n, **kw):
        st, _s, _keep = self.enqueue(n, **kw)
        return self.read(st, n)


def policy(m):
    p = Replayable()
    p.MaxInterval = m
    return p


# (E, seeds, m, first decimal seed, entities, every k-th event NMZ_NONE): every E, seed count and m of the issue;
# the large E with the small seed counts; two ranges wrap past 2^64, one crosses 999 -> 1000
CASES = [
    (1, 300, 7, 0, 1, 0),
    (2, 2049, 2**31 - 1, 990, 2, 0),
    (63, 65, 2**31, 0, 5, 7),
    (64, 2049, 2**32 + 5, 2**64 - 616, 4, 0),
    (65, 300, 2**50, 0, 16, 9),
    (255, 64, 1, 5, 3, 0),
    (256, 63, 0, 5, 40, 5),
    (257, 65, 2**31 - 1, 0, 2, 0),
    (1023, 64, 2**32 + 5, 0, 100, 11),
    (1024, 65, 2**31, 2**64 - 30, 16, 0),
    (1025, 63, 2**50, 0, 9, 13),
    (4096, 1, 7, 12345, 70, 0),
    (4096, 63, 10**8, 0, 3, 17),
    # three long segments do not fit the aligned blocks: the segment-aware compare with the two wide reductions
    (4096, 5, 2**32 + 5, 2**64 - 2, 3, 0),
    (4096, 3, 2**31, 7, 3, 17),
]


@pytest.mark.parametrize("E,S,m,lo,n_ent,none_every", CASES)
def test_sweep_stats_bit_equal(ctx, E, S, m, lo, n_ent, none_every):
    """Decimal ranges, exact and PO mode: the device stats equal the host entry point's and the restatement's for
    every seed."""
    hints, arrival, sym, entity = R.case_inputs(E, m, n_ent, none_every)
    seeds = R.decimal_seeds(lo, S)
    dl = R.delays(seeds, hints, m)
    for ent in (None, entity):
        ref = R.Ref(dl, arrival, sym, ent)
        with Plan(ctx, hints, arrival, sym, ent, m, S) as plan:
            got = plan.sweep(S, lo=lo)
        assert R.same(got, ref.stats)
        hst = R.host_delivery(seeds, hints, arrival, sym, ent, m)[0]  # the host entry point, every seed
        assert got.tobytes() == hst.tobytes()


@pytest.mark.parametrize("m", [0, 10**8, 2**31 + 11, 2**40])
def test_csr_seeds_with_the_empty_seed(ctx, m):
    seeds = ["", "foobar", "a" * 40] + [str(i) for i in range(70)]  # the empty seed is the reference's default
    hints, arrival, sym, entity = R.case_inputs(130, m, 6, 10, rng_seed=3)
    hints[5] = ""       # an empty hint
    hints[9] = hints[8]  # equal hints
    dl = R.delays(seeds, hints, m)
    for ent in (None, entity):
        ref = R.Ref(dl, arrival, sym, ent)
        with Plan(ctx, hints, arrival, sym, ent, m, len(seeds)) as plan:
            assert R.same(plan.sweep(len(seeds), seeds=seeds), ref.stats)
        r = policy(m).DeliveryOrders(hints, arrival, sym, ent, seeds=seeds, ctx=ctx)  # the host-pointer form
        assert R.same(r.stats, ref.stats)
        assert np.array_equal(r.first_equal, ref.first_equal()) and np.array_equal(r.class_rep, ref.class_rep())
        hst = R.host_delivery(seeds, hints, arrival, sym, ent, m)[0]
        assert r.stats.tobytes() == hst.tobytes()


@functools.lru_cache(maxsize=None)
def fixture(name, po):
    """A fixture of tests/golden/delivery_order_kat.json: (fx, seeds, Ref); computed once and shared, not
    modified."""
    import json
    import os
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "delivery_order_kat.json")) as f:
        fx = json.load(f)[name]
    seeds = [str(s) for s in range(fx["n_seeds"])]
    ref = R.Ref(R.delays(seeds, fx["hints"], fx["max_interval_ns"]), fx["arrival_ns"], fx["sym"],
                fx["entity"] if po else None)
    return fx, seeds, ref


def own_signatures(ctx, ref):
    """nmz_trace_signatures and nmz_unique_traces (the parent's kernels) of the delivered traces."""
    L = _lib.load()
    off, sy, en = ref.traces()
    S = len(off) - 1
    sig = np.zeros((S, 2), np.uint64)
    fe = np.zeros(S, np.uint32)
    _lib.check(L.nmz_trace_signatures(ctx.handle, _lib.ptr(off), _lib.ptr(sy), _lib.ptr(en), S, _lib.ptr(sig)))
    _lib.check(L.nmz_unique_traces(ctx.handle, _lib.ptr(off), _lib.ptr(sy), _lib.ptr(en), S, _lib.ptr(fe)))
    return sig, fe


@pytest.mark.parametrize("name,po", [("G", False), ("H", False), ("H", True)])
def test_fixture_signatures_and_classes(ctx, name, po):
    fx, seeds, ref = fixture(name, po)
    S, m = len(seeds), fx["max_interval_ns"]
    exp_fe = ref.first_equal()
    R.assert_partition_mixed(exp_fe, singletons=not po)
    want = fx["po" if po else "exact"]
    assert len(np.unique(exp_fe)) == want["n_classes"]
    ent = fx["entity"] if po else None
    with Plan(ctx, fx["hints"], fx["arrival_ns"], fx["sym"], ent, m, S) as plan:
        st, s, _ = plan.enqueue(S, lo=0)
        fe, rep, nc = plan.classes(st, S, s)
        got = Plan.read(st, S)
    assert R.same(got, ref.stats)
    # the signature is the one the project gives the delivered trace, and so are the classes
    sig, own_fe = own_signatures(ctx, ref)
    assert np.array_equal(got["sig_lo"], sig[:, 0]) and np.array_equal(got["sig_hi"], sig[:, 1])
    assert np.array_equal(fe, own_fe) and np.array_equal(fe, exp_fe)
    assert nc == want["n_classes"] and np.array_equal(rep, ref.class_rep())
    assert R.class_sizes(fe).max() == want["largest_class"]
    heads = np.nonzero(fe == np.arange(S))[0]
    assert [seeds[h] for h in heads] == [w["seed"] for w in want["heads"]]
    # the reference's literal loops (G exact, H PO: the quadratic loops stay small)
    curve = np.cumsum(fe == np.arange(S)).tolist()
    off, sy, en = ref.traces()
    G = ref.order.shape[1]
    if po:
        assert curve == O.unique_curve_po([list(zip(en[i * G:(i + 1) * G].tolist(), sy[i * G:(i + 1) * G].tolist()))
                                           for i in range(S)])
    elif name == "G":
        assert curve == O.unique_curve_exact([sy[i * G:(i + 1) * G] for i in range(S)])


def test_fixture_G_derivable_cases(ctx):
    fx, seeds, _ = fixture("G", False)
    for m in (2**19, 0):
        r = policy(m).DeliveryOrders(fx["hints"], fx["arrival_ns"], fx["sym"], seed_lo=0, n_seeds=512, ctx=ctx)
        assert r.n_classes == 1 and np.all(r.first_equal == 0)
        assert np.all(r.stats["min_gap_ns"] >= MS - m) and np.all(r.stats["n_counted"] == 6)
        if m == 0:
            assert np.all(r.stats["min_gap_ns"] == MS) and np.all(r.stats["gap_event"] == 1)
        assert r.class_rep[0] == int(np.argmax(r.stats["min_gap_ns"])) and np.all(r.class_rep[1:] == R.NONE)


def test_gap_ties_go_to_the_smaller_index(ctx):
    """Equal hints only: every seed has the same order and the same gaps, so one class whose representative is
    seed 0; with a second, seed-dependent pair the representative is the restatement's."""
    hints = ["same", "same", "twin", "twin"]
    arrival = [0, 3 * MS, 10**10, 10**10 + 5]
    sym = [11, 12, 13, 14]
    r = policy(10**8).DeliveryOrders(hints, arrival, sym, seed_lo=7, n_seeds=300, ctx=ctx)
    assert r.n_classes == 1 and r.class_rep[0] == 0 and np.all(r.stats["min_gap_ns"] == 5)
    assert np.all(r.stats["gap_event"] == 3)
    seeds = R.decimal_seeds(7, 300)
    hints2 = hints + ["x", "y"]
    arrival2 = arrival + [2 * 10**10, 2 * 10**10 + 10**7]
    sym2 = sym + [15, 16]
    ref = R.Ref(R.delays(seeds, hints2, 10**8), arrival2, sym2)
    r2 = policy(10**8).DeliveryOrders(hints2, arrival2, sym2, seed_lo=7, n_seeds=300, ctx=ctx)
    assert r2.n_classes == 2 and np.array_equal(r2.class_rep, ref.class_rep())
    assert np.array_equal(r2.first_equal, ref.first_equal())


@pytest.mark.parametrize("E,n_ent", [(65, 65), (1025, 1025), (300, 1), (1100, 65)])
def test_segment_structure(ctx, E, n_ent):
    m, S, lo = 10**8, 40, 100
    hints, arrival, sym, _ = R.case_inputs(E, m, rng_seed=5)
    seeds = R.decimal_seeds(lo, S)
    dl = R.delays(seeds, hints, m)
    if n_ent == E:  # one event per entity: nothing is compared, every seed is in one class
        entity = np.random.default_rng(1).permutation(E).astype(np.uint32)
    elif n_ent == 1:
        entity = np.full(E, 9, np.uint32)
    else:       # 65 entities of uneven sizes with NMZ_NONE mixed in
        entity = (np.random.default_rng(2).integers(0, n_ent, E) ** 2 // n_ent).astype(np.uint32)
        entity[::10] = R.NONE
    ref = R.Ref(dl, arrival, sym, entity)
    r = policy(m).DeliveryOrders(hints, arrival, sym, entity, seed_lo=lo, n_seeds=S, ctx=ctx)
    assert R.same(r.stats, ref.stats)
    assert np.array_equal(r.first_equal, ref.first_equal()) and np.array_equal(r.class_rep, ref.class_rep())
    if n_ent == E:
        assert r.n_classes == 1 and np.all(r.stats["min_gap_ns"] == R.INT64_MAX)
        assert np.all(r.stats["gap_event"] == R.NONE) and r.class_rep[0] == 0
    if n_ent == 1:  # one entity for all events is exact mode
        x = policy(m).DeliveryOrders(hints, arrival, sym, None, seed_lo=lo, n_seeds=S, ctx=ctx)
        assert x.stats.tobytes() == r.stats.tobytes()
    sig, own_fe = own_signatures(ctx, ref)
    assert np.array_equal(r.stats["sig_lo"], sig[:, 0]) and np.array_equal(r.stats["sig_hi"], sig[:, 1])
    assert np.array_equal(r.first_equal, own_fe)


def test_equal_hints_in_one_entity_give_a_constant_gap(ctx):
    hints = ["dup", "a", "dup", "b", "c"]
    arrival = [0, 10 * MS, 7 * MS, 10**12, 10**12]
    entity = [0, 1, 0, 2, 3]  # entity 0 holds the equal-hint pair; the others one event each
    r = policy(10**8).DeliveryOrders(hints, arrival, [1, 2, 3, 4, 5], entity, seed_lo=0, n_seeds=300, ctx=ctx)
    assert np.all(r.stats["min_gap_ns"] == 7 * MS) and np.all(r.stats["gap_event"] == 2) and r.n_classes == 1


def test_plan_reuse_on_two_streams_in_turn_and_argument_errors(ctx):
    import torch
    fx, seeds, ref = fixture("G", False)
    S, m = len(seeds), fx["max_interval_ns"]
    with Plan(ctx, fx["hints"], fx["arrival_ns"], fx["sym"], None, m, S) as plan:
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        a, _, _ = plan.enqueue(S, lo=0, stream=s1)
        s1.synchronize()
        b, _, _ = plan.enqueue(100, lo=50, stream=s2)
        s2.synchronize()
        c, _, _ = plan.enqueue(S, lo=0, stream=s1)
        assert R.same(Plan.read(a, S), ref.stats) and R.same(Plan.read(b, 100), ref.stats[50:150])
        assert Plan.read(c, S).tobytes() == Plan.read(a, S).tobytes()
        plan.sweep(0, lo=0)  # no seeds: nothing to do
        with pytest.raises(_lib.NmzInvalidArgument, match="more seeds than the plan"):
            plan.sweep(S + 1, lo=0)
    r = policy(m).DeliveryOrders(fx["hints"], fx["arrival_ns"], fx["sym"], seeds=[], ctx=ctx)
    assert len(r.stats) == 0 and r.n_classes == 0 and r.representatives() == []
    with pytest.raises(_lib.NmzInvalidArgument, match=r"n_events must be in \[1, 4096\]"):
        Plan(ctx, [], [], [], None, m, 10)
    with pytest.raises(_lib.NmzInvalidArgument, match="at most 2\\^32-1 seeds"):
        Plan(ctx, fx["hints"], fx["arrival_ns"], fx["sym"], None, m, 2**32)
    with pytest.raises(ValueError, match="either seeds or seed_lo"):
        policy(m).DeliveryOrders(fx["hints"], fx["arrival_ns"], fx["sym"], ctx=ctx)


def test_recorded_and_predicted_signatures_class_together(ctx):
    """nmz_sig_classes_dev over recorded + predicted signatures: a recorded run that delivered seed s's order lands
    in seed s's class."""
    import torch
    fx, seeds, ref = fixture("H", True)
    S, m = len(seeds), fx["max_interval_ns"]
    picks = [3, 500, 2048]
    off, sy, en = ref.traces()
    G = ref.order.shape[1]
    roff = np.arange(len(picks) + 1, dtype=np.uint64) * np.uint64(G)
    rsy = np.concatenate([sy[p * G:(p + 1) * G] for p in picks])
    ren = np.concatenate([en[p * G:(p + 1) * G] for p in picks])
    rsig = np.zeros((len(picks), 2), np.uint64)
    L = _lib.load()
    _lib.check(L.nmz_trace_signatures(ctx.handle, _lib.ptr(roff), _lib.ptr(rsy), _lib.ptr(ren), len(picks),
                                      _lib.ptr(rsig)))
    r = policy(m).DeliveryOrders(fx["hints"], fx["arrival_ns"], fx["sym"], fx["entity"], seed_lo=0, n_seeds=S, ctx=ctx)
    psig = np.stack([r.stats["sig_lo"], r.stats["sig_hi"]], axis=1)
    both = torch.from_numpy(np.concatenate([rsig, psig]).view(np.int64)).cuda()
    n = len(picks) + S
    fe = torch.zeros(n, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    _lib.check(L.nmz_sig_classes_dev(ctx.handle, _vp(both), n, _vp(fe), None))
    torch.cuda.synchronize()
    fe = fe.cpu().numpy().view(np.uint32)
    exp_fe = ref.first_equal()
    for i, p in enumerate(picks):
        members = np.nonzero(fe == fe[i])[0]
        assert fe[i] <= i and len(picks) + p in members
        assert set(members[members >= len(picks)] - len(picks)) == set(np.nonzero(exp_fe == exp_fe[p])[0])
    # and the recorded signatures drop those classes from the seeds worth replaying
    reps = r.representatives(known_sigs=rsig)
    assert len(reps) == r.n_classes - len({int(exp_fe[p]) for p in picks})
    assert not {int(exp_fe[x]) for x in reps} & {int(exp_fe[p]) for p in picks}
