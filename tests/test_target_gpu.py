"""GPU: the nearest-order sweep (nmz_replayable_target_*; csrc/target.hip) against nmz_replayable_target_host, the
numpy restatement over the C oracle's delays (tests/target_ref.py), the FNV-only known answers
(tests/golden/target_order_kat.json) and the delivery sweep's signatures. Everything is integer: every comparison is
equality. No test depends on a rate."""
import ctypes
import functools
import json
import os

import numpy as np
import pytest

import delivery_ref as R
import target_ref as T
from namazu_amd import _lib, replay
from namazu_amd.explorepolicy import Replayable
from oracle import oracle as O

pytestmark = pytest.mark.gpu
MS = R.MS
NONE = R.NONE
PAIRS, PREFIX = _lib.NMZ_TARGET_RANK_PAIRS, _lib.NMZ_TARGET_RANK_PREFIX


def _vp(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


class Plan:
    """nmz_replayable_target_plan over one trace and target; sweeps into torch device buffers."""

    def __init__(self, ctx, hints, arrival, entity, tp, m, max_seeds):
        self.L, self.ctx = _lib.load(), ctx
        ho, hb = O.to_csr(list(hints))
        arr = np.ascontiguousarray(arrival, np.int64)
        t = np.ascontiguousarray(tp, np.uint32)
        en = None if entity is None else np.ascontiguousarray(entity, np.uint32)
        self.h = ctypes.c_void_p()
        _lib.check(self.L.nmz_replayable_target_plan_create(ctx.handle, _lib.ptr(ho), _lib.ptr(hb), len(hints), m,
                                                            _lib.ptr(arr), _lib.ptr(en), _lib.ptr(t), max_seeds,
                                                            ctypes.byref(self.h)))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        _lib.check(self.L.nmz_replayable_target_plan_destroy(self.h))

    def info(self):
        out = np.zeros(2, np.uint32)
        _lib.check(self.L.nmz_replayable_target_plan_info(self.h, _lib.ptr(out[0:1]), _lib.ptr(out[1:2])))
        return int(out[0]), int(out[1])

    def enqueue(self, n, lo=None, seeds=None, seed0=0, k=0, mode=PAIRS, want_stats=True, stream=None):
        import torch
        st = torch.zeros(max(n, 1) * 24, dtype=torch.uint8, device="cuda") if want_stats else None
        tk = torch.zeros(max(k, 1) * 24, dtype=torch.uint8, device="cuda") if k else None
        # the buffers' zeroing ran on torch's current stream; the sweep runs on `stream`, or (torch's default stream
        # handle is NULL) on the context's own stream
        torch.cuda.current_stream().synchronize()
        s = ctypes.c_void_p((stream or torch.cuda.current_stream()).cuda_stream)
        if seeds is None:
            _lib.check(self.L.nmz_replayable_target_sweep_decimal_dev(self.h, lo, n, mode, k, _vp(st), _vp(tk), s))
            keep = ()
        else:
            so, sb = O.to_csr(seeds)
            keep = (torch.from_numpy(so.view(np.int32)).cuda(), torch.from_numpy(sb).cuda())
            torch.cuda.current_stream().synchronize()
            _lib.check(self.L.nmz_replayable_target_sweep_dev(self.h, _vp(keep[0]), _vp(keep[1]), n, seed0, mode, k,
                                                              _vp(st), _vp(tk), s))
        return st, tk, keep

    @staticmethod
    def read(st, n):
        import torch
        torch.cuda.synchronize()
        return np.frombuffer(st.cpu().numpy().tobytes(), _lib.TARGET_STATS_DTYPE)[:n]

    @staticmethod
    def read_topk(tk, k):
        import torch
        torch.cuda.synchronize()
        return np.frombuffer(tk.cpu().numpy().tobytes(), _lib.TOPK_DTYPE)[:k]

    def sweep(self, n, **kw):
        st, _tk, _keep = self.enqueue(n, **kw)
        return self.read(st, n)


def policy(m):
    p = Replayable()
    p.MaxInterval = m
    return p


def make_target(kind, dl, arrival, E, S):
    """own: the order of seed index 1 (0 when there is one seed); reverse: that reversed; random: a permutation;
    sparse: own without every 5th event, at positions 7 i + 3."""
    own = R.Ref(dl[min(1, S - 1):min(1, S - 1) + 1], arrival, np.zeros(E, np.uint64)).order[0]
    if kind == "own":
        return T.target_of_order(own, E)
    if kind == "reverse":
        return T.target_of_order(own[::-1], E)
    if kind == "random":
        return T.target_of_order(np.random.default_rng(E).permutation(E), E)
    return T.target_of_order(np.array([e for e in own if e % 5 != 4], np.int64), E, stride=7, offset=3)


# (E, seeds, m, first decimal seed, entities, every k-th event NMZ_NONE, target): every shape and m of the issue; two
# ranges wrap past 2^64, one crosses 999 -> 1000; the targets rotate (the reverse and the random one drive the long
# merges and the width of the sum, the sparse one the absent events)
CASES = [
    (1, 300, 7, 0, 1, 0, "own"),
    (2, 2049, 2**31 - 1, 990, 2, 0, "reverse"),
    (3, 65, 1, 0, 2, 0, "own"),
    (63, 65, 2**31, 0, 5, 7, "random"),
    (64, 2049, 2**32 + 5, 2**64 - 616, 4, 0, "own"),
    (65, 300, 2**50, 0, 16, 9, "sparse"),
    (255, 64, 10**8, 5, 3, 0, "reverse"),
    (256, 63, 0, 5, 40, 5, "random"),
    (257, 65, 2**31 - 1, 0, 2, 0, "own"),
    (1023, 64, 2**32 + 5, 0, 100, 11, "sparse"),
    (1024, 65, 2**31, 2**64 - 30, 16, 0, "random"),
    (1025, 63, 2**50, 0, 9, 13, "reverse"),
    # three long segments do not fit the aligned blocks: the segment-aware compare, the largest LDS footprint
    (4096, 63, 10**8, 0, 3, 17, "own"),
    (4096, 5, 2**32 + 5, 2**64 - 2, 3, 0, "random"),
]


@pytest.mark.parametrize("E,S,m,lo,n_ent,none_every,kind", CASES)
def test_sweep_stats_bit_equal(ctx, E, S, m, lo, n_ent, none_every, kind):
    """Decimal ranges, exact and PO mode: the device stats equal the host entry point's and the restatement's for
    every seed."""
    hints, arrival, _sym, entity = R.case_inputs(E, m, n_ent, none_every)
    seeds = R.decimal_seeds(lo, S)
    dl = R.delays(seeds, hints, m)
    tp = make_target(kind, dl, arrival, E, S)
    for ent in (None, entity):
        ref = T.TRef(dl, arrival, tp, ent)
        if kind in ("reverse", "random") and E >= 63 and m:
            assert int(ref.stats["n_discordant"].max()) > ref.n_pairs // 4, "degenerate input"
        with Plan(ctx, hints, arrival, ent, tp, m, S) as plan:
            got = plan.sweep(S, lo=lo)
            assert plan.info() == (ref.n_counted, ref.n_pairs)
        assert R.same(got, ref.stats)
        hst = T.host_target(seeds, hints, arrival, ent, tp, m)[0]  # the host entry point, every seed
        assert got.tobytes() == hst.tobytes()


@pytest.mark.parametrize("E,S,n_ent", [(1100, 9, 65), (300, 33, 1)])
def test_segment_structure(ctx, E, S, n_ent):
    """65 entities of uneven sizes (one long segment among many short ones) and one entity plus NMZ_NONE events,
    which is exact mode over the counted events. The aligned layout is what the cases above with many entities of
    like sizes take."""
    m, lo = 10**8, 100
    hints, arrival, _sym, _ = R.case_inputs(E, m, rng_seed=5)
    seeds = R.decimal_seeds(lo, S)
    dl = R.delays(seeds, hints, m)
    if n_ent == 1:
        entity = np.full(E, 9, np.uint32)
    else:
        entity = (np.random.default_rng(2).integers(0, n_ent, E) ** 2 // n_ent).astype(np.uint32)
    entity[::10] = NONE
    for kind in ("own", "random"):
        tp = make_target(kind, dl, arrival, E, S)
        ref = T.TRef(dl, arrival, tp, entity)
        r = policy(m).NearestOrders(hints, arrival, target_pos=tp, entity=entity, seed_lo=lo, n_seeds=S, ctx=ctx)
        assert R.same(r.stats, ref.stats) and (r.n_counted, r.n_pairs) == (ref.n_counted, ref.n_pairs)
        assert r.stats.tobytes() == T.host_target(seeds, hints, arrival, entity, tp, m)[0].tobytes()
        if n_ent == 1:  # one entity for the counted events is exact mode over them
            tpx = np.where(entity == NONE, NONE, tp).astype(np.uint32)
            x = policy(m).NearestOrders(hints, arrival, target_pos=tpx, seed_lo=lo, n_seeds=S, ctx=ctx)
            assert x.stats.tobytes() == r.stats.tobytes()


@pytest.mark.parametrize("m", [0, 10**8, 2**31 + 11, 2**40])
def test_csr_seeds_with_the_empty_seed(ctx, m):
    seeds = ["", "foobar", "a" * 40] + [str(i) for i in range(70)]  # the empty seed is the reference's default
    hints, arrival, _sym, entity = R.case_inputs(130, m, 6, 10, rng_seed=3)
    hints[5] = ""        # an empty hint
    hints[9] = hints[8]  # equal hints
    dl = R.delays(seeds, hints, m)
    tp = make_target("sparse", dl, arrival, 130, len(seeds))
    for ent in (None, entity):
        ref = T.TRef(dl, arrival, tp, ent)
        with Plan(ctx, hints, arrival, ent, tp, m, len(seeds)) as plan:
            assert R.same(plan.sweep(len(seeds), seeds=seeds), ref.stats)
        r = policy(m).NearestOrders(hints, arrival, target_pos=tp, entity=ent, seeds=seeds, ctx=ctx)  # host pointers
        assert R.same(r.stats, ref.stats)
        assert r.stats.tobytes() == T.host_target(seeds, hints, arrival, ent, tp, m)[0].tobytes()


@functools.lru_cache(maxsize=None)
def kat(name):
    """A fixture of tests/golden/target_order_kat.json with its restatement: (fx, seeds, TRef); computed once and
    shared, not modified."""
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "target_order_kat.json")) as f:
        fx = json.load(f)[name]
    seeds = [str(s) for s in range(fx["n_seeds"])]
    ref = T.TRef(R.delays(seeds, fx["hints"], fx["max_interval_ns"]), fx["arrival_ns"], fx["target_pos"],
                 fx.get("entity"))
    return fx, seeds, ref


@functools.lru_cache(maxsize=None)
def wide_case():
    """400 events (79,800 pairs, past the 16 bits of the selection's coarse key) x 600 decimal seeds that wrap past
    2^64, the target one seed's own order; computed once and shared, not modified."""
    E, S, m, lo = 400, 600, 10**8, 2**64 - 300
    hints, arrival, _sym, _ = R.case_inputs(E, m)
    seeds = R.decimal_seeds(lo, S)
    dl = R.delays(seeds, hints, m)
    tp = make_target("own", dl, arrival, E, S)
    return hints, arrival, tp, seeds, T.TRef(dl, arrival, tp, None), m, lo


def entries(tk):
    return [{k: int(e[k]) for k in ("seed", "sum_delay_ns", "n_fault", "first_fault")} for e in tk]


@pytest.mark.parametrize("name", ["G", "H"])
def test_known_answers_through_the_kernel(ctx, name):
    fx, seeds, ref = kat(name)
    S = len(seeds)
    p = policy(fx["max_interval_ns"])
    r = p.NearestOrders(fx["hints"], fx["arrival_ns"], target_order=fx["target_order"], entity=fx.get("entity"),
                        seed_lo=0, n_seeds=S, k=8, ctx=ctx)
    assert (r.n_counted, r.n_pairs) == (fx["n_counted"], fx["n_pairs"])
    for f in ("n_discordant", "prefix_len", "n_in_place", "min_gap_ns"):
        assert r.stats[f].tolist() == fx[f], f
    assert R.same(r.stats, ref.stats)
    assert entries(r.topk) == fx["top8_pairs"]
    r2 = p.NearestOrders(fx["hints"], fx["arrival_ns"], target_pos=fx["target_pos"], entity=fx.get("entity"),
                         seeds=seeds, k=8, rank_by="prefix", want_stats=False, ctx=ctx)
    assert r2.stats is None and entries(r2.topk) == fx["top8_prefix"]


@pytest.mark.parametrize("name", ["G", "H"])
def test_zero_discordant_is_the_target_seeds_delivery_class(ctx, name):
    """n_discordant == 0 exactly for the seeds whose DeliveryOrders signature equals the target seed's."""
    fx, seeds, ref = kat(name)
    S, ent = len(seeds), fx.get("entity")
    p = policy(fx["max_interval_ns"])
    r = p.NearestOrders(fx["hints"], fx["arrival_ns"], target_pos=fx["target_pos"], entity=ent, seed_lo=0,
                        n_seeds=S, ctx=ctx)
    sym = np.arange(1, len(fx["hints"]) + 1, dtype=np.uint64) * np.uint64(0x9e3779b97f4a7c15)  # distinct symbols
    d = p.DeliveryOrders(fx["hints"], fx["arrival_ns"], sym, ent, seed_lo=0, n_seeds=S, ctx=ctx)
    t = int(fx["target_seed"])
    same_class = d.first_equal == d.first_equal[t]
    assert 1 < same_class.sum() < S
    assert np.array_equal(r.stats["n_discordant"] == 0, same_class)
    assert np.array_equal(r.stats["prefix_len"] == r.n_counted, same_class)


@pytest.mark.parametrize("k", [1, 8, 64, 256])
@pytest.mark.parametrize("mode,rank_by", [(PAIRS, "pairs"), (PREFIX, "prefix")])
def test_topk_equals_a_sort_of_the_stats(ctx, k, mode, rank_by):
    """The 6-event fixture: many seeds share n_discordant (and the prefix mode's first two fields), so ties are
    decided by min_gap_ns and then by the smaller seed; and a 257-event trace whose counts pass the coarse key's
    16 bits."""
    fx, seeds, ref = kat("G")
    S = len(seeds)
    keys = [(int(s["n_discordant"]), int(s["prefix_len"])) for s in ref.stats]
    assert len(set(keys)) < S // 8, "degenerate input: no ties on the leading fields"
    with Plan(ctx, fx["hints"], fx["arrival_ns"], None, fx["target_pos"], fx["max_interval_ns"], S) as plan:
        st, tk, _ = plan.enqueue(S, lo=0, k=k, mode=mode)
        got = Plan.read_topk(tk, k)
        assert R.same(Plan.read(st, S), ref.stats)
        assert got.tobytes() == T.topk(ref.stats, ref.n_pairs, range(S), k, rank_by).tobytes()
        _, tk2, _ = plan.enqueue(S, lo=0, k=k, mode=mode, want_stats=False)  # d_stats == NULL: the same list
        assert Plan.read_topk(tk2, k).tobytes() == got.tobytes()
    hints, arrival, tp, seeds, ref, m, lo = wide_case()
    S = len(seeds)
    assert ref.n_pairs - int(ref.stats["n_discordant"].max()) > 0xffff
    with Plan(ctx, hints, arrival, None, tp, m, S) as plan:
        _, tk, _ = plan.enqueue(S, lo=lo, k=k, mode=mode, want_stats=False)
        want = T.topk(ref.stats, ref.n_pairs, [int(s) for s in seeds], k, rank_by)
        assert Plan.read_topk(tk, k).tobytes() == want.tobytes()


def test_topk_orders_min_gap_over_its_range(ctx):
    """sum_delay_ns = min_gap_ns from 0 to 2^51 and INT64_MAX: the selection's coarse key (the top 48 bits of the
    sign-flipped value) must keep that order. E = 1 gives INT64_MAX for every seed; two events 2^50 apart with
    m = 2^50 give gaps up to 2^51; equal arrivals give gaps from 0 up."""
    r = policy(10**8).NearestOrders(["only"], [5], target_order=[0], seed_lo=0, n_seeds=300, k=8, ctx=ctx)
    assert np.all(r.stats["min_gap_ns"] == R.INT64_MAX) and np.all(r.stats["gap_event"] == NONE)
    assert (r.n_counted, r.n_pairs) == (1, 0) and np.all(r.stats["prefix_len"] == 1)
    assert r.topk.tobytes() == T.topk(r.stats, 0, range(300), 8, "pairs").tobytes()
    assert r.topk["seed"].tolist() == list(range(8)) and np.all(r.topk["sum_delay_ns"] == R.INT64_MAX)
    S = 3000
    for arrival in ([0, 2**50], [7, 7]):
        p = policy(2**50)
        # hints of different lengths: the two delays are then unrelated (one-byte hints differ by a few multiples
        # of the FNV prime for every seed)
        r = p.NearestOrders(["first:event", "second"], arrival, target_order=[0, 1], seed_lo=0, n_seeds=S, k=256,
                            ctx=ctx)
        gaps = r.stats["min_gap_ns"]
        assert gaps.min() >= 0 and len(np.unique(gaps >> 16)) > 256  # the coarse key sees many values
        if arrival[0] == 0:
            assert gaps.max() > 2**50
        assert r.topk.tobytes() == T.topk(r.stats, 1, range(S), 256, "pairs").tobytes()


def test_merged_lists_of_two_ranges_equal_one_sweep(ctx):
    import torch
    fx, seeds, ref = kat("H")
    S, k = len(seeds), 64
    L = _lib.load()
    with Plan(ctx, fx["hints"], fx["arrival_ns"], fx["entity"], fx["target_pos"], fx["max_interval_ns"], S) as plan:
        for mode, rank_by in ((PAIRS, "pairs"), (PREFIX, "prefix")):
            _, whole, _ = plan.enqueue(S, lo=0, k=k, mode=mode, want_stats=False)
            whole = Plan.read_topk(whole, k)
            _, a, _ = plan.enqueue(200, lo=0, k=k, mode=mode, want_stats=False)
            a = Plan.read_topk(a, k)
            _, b, _ = plan.enqueue(S - 200, lo=200, k=k, mode=mode, want_stats=False)
            b = Plan.read_topk(b, k)
            lists = torch.from_numpy(np.frombuffer(a.tobytes() + b.tobytes(), np.uint8).copy()).cuda()
            scratch = torch.zeros_like(lists)
            out = torch.zeros(k * 24, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            _lib.check(L.nmz_topk_merge_dev(ctx.handle, _vp(lists), 2, k, _vp(scratch), _vp(out), None))
            assert Plan.read_topk(out, k).tobytes() == whole.tobytes()
            assert whole.tobytes() == T.topk(ref.stats, ref.n_pairs, range(S), k, rank_by).tobytes()


def test_csr_topk_seed_is_seed0_plus_the_index(ctx):
    fx, seeds, ref = kat("G")
    with Plan(ctx, fx["hints"], fx["arrival_ns"], None, fx["target_pos"], fx["max_interval_ns"], 100) as plan:
        _, tk, _ = plan.enqueue(100, seeds=seeds[:100], seed0=2**64 - 5, k=8)
        want = T.topk(ref.stats[:100], ref.n_pairs, [(2**64 - 5 + i) % 2**64 for i in range(100)], 8, "pairs")
        assert Plan.read_topk(tk, 8).tobytes() == want.tobytes()
        # fewer seeds than k: sentinels past them
        _, tk, _ = plan.enqueue(3, lo=0, k=8)
        got = Plan.read_topk(tk, 8)
        assert got.tobytes() == T.topk(ref.stats[:3], ref.n_pairs, range(3), 8, "pairs").tobytes()
        assert got[3:].tolist() == [T.SENTINEL] * 5


def test_nearest_orders_to_a_replay(ctx):
    """NearestOrders -> replay.replayable_seeds -> replay_env on the 6-event fixture: the best seed reproduces the
    recorded order (and the host check agrees), and the environment carries it."""
    fx, seeds, _ = kat("G")
    p = policy(fx["max_interval_ns"])
    r = p.NearestOrders(fx["hints"], fx["arrival_ns"], target_order=fx["target_order"], seeds=seeds, k=8,
                        want_stats=False, ctx=ctx)
    best = replay.replayable_seeds(r.topk, seeds)
    assert best == [str(e["seed"]) for e in fx["top8_pairs"]] and fx["target_seed"] in best
    env = replay.replay_env(best[0], {"PATH": "/bin"})
    assert env == {"PATH": "/bin", "NMZ_REPLAY_SEED": best[0]}
    p.Seed = env["NMZ_REPLAY_SEED"]
    st, n_counted, _ = p.target_distance(fx["hints"], fx["arrival_ns"], fx["target_pos"])
    assert int(st["n_discordant"]) == 0 and int(st["prefix_len"]) == n_counted == 6
    order, _, _ = p.delivery_order(fx["hints"], fx["arrival_ns"], np.zeros(6, np.uint64))
    assert order.tolist() == fx["target_order"]


def test_plan_reuse_on_two_streams_in_turn_and_argument_errors(ctx):
    import torch
    fx, seeds, ref = kat("G")
    S, m = len(seeds), fx["max_interval_ns"]
    hints, arrival, tp = fx["hints"], fx["arrival_ns"], fx["target_pos"]
    with Plan(ctx, hints, arrival, None, tp, m, S) as plan:
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        a, ta, _ = plan.enqueue(S, lo=0, k=8, stream=s1)
        s1.synchronize()
        b, _, _ = plan.enqueue(100, lo=50, stream=s2)
        s2.synchronize()
        c, tc, _ = plan.enqueue(S, lo=0, k=8, stream=s1)
        assert R.same(Plan.read(a, S), ref.stats) and R.same(Plan.read(b, 100), ref.stats[50:150])
        assert Plan.read(c, S).tobytes() == Plan.read(a, S).tobytes()
        assert Plan.read_topk(tc, 8).tobytes() == Plan.read_topk(ta, 8).tobytes()
        plan.enqueue(0, lo=0)  # no seeds: nothing to do
        with pytest.raises(_lib.NmzInvalidArgument, match="more seeds than the plan"):
            plan.sweep(S + 1, lo=0)
        with pytest.raises(_lib.NmzInvalidArgument, match="rank_mode must be NMZ_TARGET_RANK_PAIRS or"):
            plan.enqueue(S, lo=0, k=8, mode=2)
        with pytest.raises(_lib.NmzInvalidArgument, match="top-k supports k <= 256"):
            plan.enqueue(S, lo=0, k=257)
        with pytest.raises(_lib.NmzInvalidArgument, match="d_stats is NULL and k is 0"):
            plan.enqueue(S, lo=0, want_stats=False)
        with pytest.raises(_lib.NmzInvalidArgument, match="d_topk is NULL"):
            _lib.check(plan.L.nmz_replayable_target_sweep_decimal_dev(plan.h, 0, S, PAIRS, 8, _vp(a), None, None))
    r = policy(m).NearestOrders(hints, arrival, target_pos=tp, seeds=[], k=4, ctx=ctx)
    assert len(r.stats) == 0 and r.topk.tolist() == [T.SENTINEL] * 4
    with pytest.raises(_lib.NmzInvalidArgument, match=r"n_events must be in \[1, 4096\]"):
        Plan(ctx, [], [], None, [], m, 10)
    with pytest.raises(_lib.NmzInvalidArgument, match="at most 2\\^32-1 seeds"):
        Plan(ctx, hints, arrival, None, tp, m, 2**32)
    with pytest.raises(_lib.NmzInvalidArgument, match="target_pos 2 appears twice among the counted events"):
        Plan(ctx, hints, arrival, None, [0, 1, 2, 2, 4, 5], m, 10)
    with pytest.raises(_lib.NmzInvalidArgument, match=r"max_interval_ns must be in \[0, 2\^50\]"):
        Plan(ctx, hints, arrival, None, tp, 2**50 + 1, 10)
    with pytest.raises(_lib.NmzInvalidArgument, match=r"arrival_ns\[0\] must be in \[0, 2\^50\]"):
        Plan(ctx, hints, [-1] + arrival[1:], None, tp, m, 10)
    with pytest.raises(_lib.NmzInvalidArgument, match=r"entity\[5\] must be < 16384 or NMZ_NONE"):
        Plan(ctx, hints, arrival, [0, 0, 0, 0, 0, 16384], tp, m, 10)
    ho, hb = O.to_csr(hints)
    arr, tpa, st = np.asarray(arrival, np.int64), np.asarray(tp, np.uint32), np.zeros(4, _lib.TARGET_STATS_DTYPE)
    with pytest.raises(_lib.NmzInvalidArgument, match="rank_mode must be"):
        _lib.check(_lib.load().nmz_replayable_target_sweep_decimal(
            ctx.handle, 0, 4, _lib.ptr(ho), _lib.ptr(hb), 6, m, _lib.ptr(arr), None, _lib.ptr(tpa), 7, 0,
            _lib.ptr(st), None, None, None))
    with pytest.raises(ValueError, match="either seeds or seed_lo"):
        policy(m).NearestOrders(hints, arrival, target_pos=tp, ctx=ctx)


def test_nothing_counted_and_zero_interval_fill_one_record(ctx):
    hints, arrival, _sym, entity = R.case_inputs(64, 10**8, 4, 0)
    r = policy(10**8).NearestOrders(hints, arrival, target_pos=np.full(64, NONE, np.uint32), seed_lo=0, n_seeds=300,
                                    k=4, ctx=ctx)
    assert (r.n_counted, r.n_pairs) == (0, 0) and r.stats.tolist() == [(0, 0, R.INT64_MAX, NONE, 0)] * 300
    assert r.topk["seed"].tolist() == [0, 1, 2, 3]
    tp = T.target_of_order(np.random.default_rng(1).permutation(64), 64)
    r = policy(0).NearestOrders(hints, arrival, target_pos=tp, entity=entity, seed_lo=5, n_seeds=300, ctx=ctx)
    hst = T.host_target(["5"], hints, arrival, entity, tp, 0)[0]
    assert r.stats.tobytes() == hst.tobytes() * 300 and int(hst[0]["n_discordant"]) > 0
