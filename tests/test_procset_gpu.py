"""GPU: ProcSetEvent decisions (nmz_procset_sweep, nmz_procset_decide) against the plain-Python reference
(tests/procset_ref.py over the oracle's Go generator). Everything is integer: every comparison is equality."""
import ctypes
import functools

import numpy as np
import pytest

import procset_ref as R
from namazu_amd import _lib
from namazu_amd.explorepolicy import Random
from oracle import oracle as O

pytestmark = pytest.mark.gpu

POLICIES = ["mild", "extreme", "dirichlet"]
RANGED = (30_000_000, 100_000_000)
FIXED = (5_000_000, 5_000_000)
WIDE = (0, 2**62 + 1)  # Int63n rejects about half of the delay draws: the sub-policy's first output index varies
RNG = np.random.default_rng(20260)


def policy(name, interval=RANGED, use_batch=True, prioritized=3, reset_probability=0.1, seed=0):
    p = Random()
    p.MinInterval, p.MaxInterval = interval
    p.ProcPolicy = name
    p.PPPMild.UseBatch, p.PPPExtreme.Prioritized, p.PPPDirichlet.ResetProbability = use_batch, prioritized, \
        reset_probability
    p.Seed = seed
    ref = R.Params(POLICIES.index(name), use_batch, prioritized, reset_probability)
    return p, O.random_params(interval[0], interval[1], 0.0), ref


def same_attrs(got, exp):
    return np.array_equal(np.asarray(got).astype(R.ATTR_DTYPE), exp)


def same_stats(got, exp):
    return np.array_equal(np.asarray(got).astype(R.STATS_DTYPE), exp)


def same_topk(got, exp):
    return np.array_equal(np.asarray(got).astype(R.TOPK_DTYPE), exp)


# ---- the sweep against the reference: 4,096 consecutive seeds (a wave carries ~16 seeds of one bucket) over 12 events
N_SEEDS, SEED0 = 4096, 77_000
N_PROCS = [1, 2, 40, 64, 65, 7, 410, 3, 512, 16, 0, 5]  # powers of two (Go's mask path), odd sizes, both caps' side
EVHASH = RNG.integers(0, 2**64, size=len(N_PROCS), dtype=np.uint64)
EVCLASS = np.array([0, 1, 0, 1, 1, 0, 0, 1, 1, 0, 0, 1], np.uint8)  # both entity classes
NONE = _lib.NMZ_NONE
TARGET = [0, 1, 39, NONE, 64, NONE, 409, 2, 300, NONE, NONE, 4]  # a valid slot on eight events


def sweep_case(name):
    n_procs = np.array(N_PROCS, np.uint32)
    if name != "mild":
        n_procs[10] = 9  # the zero-process event is for mild only
    return n_procs, np.array(TARGET, np.uint32)


@functools.lru_cache(maxsize=None)
def sweep_reference(name):
    """Computed once per policy and shared; the arrays are not modified."""
    _, rp, ref = policy(name)
    n_procs, target = sweep_case(name)
    return R.sweep(SEED0, N_SEEDS, EVHASH, EVCLASS, n_procs, target, rp, ref, n_dump=3)


@pytest.mark.parametrize("name", POLICIES)
def test_sweep_matches_reference(ctx, name):
    p, _, _ = policy(name)
    n_procs, target = sweep_case(name)
    st, dl, at, _ = sweep_reference(name)
    for desc in (True, False):
        r = p.ProcSetSweep(SEED0, N_SEEDS, EVHASH, EVCLASS, n_procs, target, n_dump=3, k=8, descending=desc, ctx=ctx)
        assert same_stats(r.stats, st)
        assert np.array_equal(r.delays, dl) and same_attrs(r.attrs, at)
        assert same_topk(r.topk, R.topk(st, SEED0, 8, desc))
    assert np.all(r.stats["flags"] == 0)


def test_topk_ties(ctx):
    """mild with one process and a target: 40 distinct scores over 4,096 seeds, so the top-k is decided by the seed."""
    p, rp, ref = policy("mild")
    eh, ec, n, t = EVHASH[:1], EVCLASS[:1], np.array([1], np.uint32), np.array([0], np.uint32)
    st, _, _, _ = R.sweep(SEED0, 600, eh, ec, n, t, rp, ref)
    for desc in (True, False):
        r = p.ProcSetSweep(SEED0, 600, eh, ec, n, t, k=256, descending=desc, ctx=ctx)
        assert same_stats(r.stats, st)
        assert same_topk(r.topk, R.topk(st, SEED0, 256, desc))
    assert len(set(r.topk["target_score"].tolist())) < 40


# ---- forced re-draws: the rare branch of the sweep kernel (statistics path only, no dump), then nmz_procset_decide
def rejection_groups(golden):
    """(id, policy kwargs, interval, hits [(evhash, n_procs)], seed)"""
    g = golden("procset_rejections.json")
    out = []
    for case in sorted({v["case"] for v in g["vectors"]}):
        vs = [v for v in g["vectors"] if v["case"] == case]
        v = vs[0]
        out.append((case, dict(name=v["policy"], use_batch=bool(v["use_batch"]), prioritized=v["prioritized"],
                               reset_probability=v["reset_probability"]), (v["min_ns"], v["max_ns"]),
                    [(x["evhash"], x["n_procs"]) for x in vs], g["seed"]))
    g = golden("random_rejections.json")
    for kind, interval in (("fixed", FIXED), ("ranged", RANGED)):
        # the vectors reject the first Intn(999) after the delay draw: dirichlet's first draw, and extreme's first
        # mark draw for 410 processes (2^31 mod 410 = 408 >= 281 = 2^31 mod 999)
        out.append((f"k2_{kind}_dirichlet", dict(name="dirichlet"), interval, [(h, 5) for h in g[kind]], g["seed"]))
        out.append((f"k2_{kind}_extreme", dict(name="extreme"), interval, [(h, 410) for h in g[kind]], g["seed"]))
        if kind == "fixed":  # the first fixed vector rejects mild's Int31n(40) as well
            out.append((f"k2_{kind}_mild", dict(name="mild"), interval, [(h, 5) for h in g[kind]], g["seed"]))
    return out


GROUP_IDS = ["dirichlet_mid", "extreme_mark", "extreme_prio", "mild_mid", "k2_fixed_dirichlet", "k2_fixed_extreme",
             "k2_fixed_mild", "k2_ranged_dirichlet", "k2_ranged_extreme"]


@pytest.mark.parametrize("gid", GROUP_IDS)
def test_rejected_draws(ctx, golden, gid):
    _, kw, interval, hits, seed = next(g for g in rejection_groups(golden) if g[0] == gid)
    p, rp, ref = policy(interval=interval, seed=seed, **kw)
    fill = RNG.integers(0, 2**64, size=9, dtype=np.uint64)
    hh = np.array([h for h, _ in hits], np.uint64)
    hn = [n for _, n in hits]
    eh = np.concatenate([fill[:3], hh, fill[3:6], hh, fill[6:]])
    n_procs = np.array([3, 17, 1] + hn + [8, 5, 2] + hn + [4, 33, 6], np.uint32)
    ec = np.zeros(len(eh), np.uint8)
    ec[3 + len(hits) + 3:3 + 2 * len(hits) + 3] = 1  # second copy prioritized
    target = np.where(np.arange(len(eh)) % 2 == 0, n_procs - 1, NONE).astype(np.uint32)
    seed0 = seed - 100
    st, _, _, outs = R.sweep(seed0, 201, eh, ec, n_procs, target, rp, ref)
    r = p.ProcSetSweep(seed0, 201, eh, ec, n_procs, target, k=8, ctx=ctx)  # no dump: statistics path only
    assert same_stats(r.stats, st)
    assert same_topk(r.topk, R.topk(st, seed0, 8, True))
    # the same inputs through nmz_procset_decide, for the vectors' seed
    dl, at = R.decide_events(seed, eh, ec, n_procs, rp, ref)
    d, a, _ = _decide(ctx, p, eh, ec, n_procs)
    assert np.array_equal(d, dl) and same_attrs(a, at)
    # the vectors' first copies do take a re-draw for their seed: one output more than the decision has draws
    # (of the K2 vectors only some reject mild's Int31n(40) too)
    took = []
    for j in range(len(hits)):
        e = 3 + j
        _, a1, _, _, n_out = R.decide(seed, int(eh[e]), 0, int(n_procs[e]), rp, ref)
        assert n_out == outs[100, e]
        took.append(n_out == R.draws(int(n_procs[e]), rp, ref, 0, a1) + 1)
    assert any(took) if gid.endswith("_mild") and gid.startswith("k2_") else all(took)


def _decide(ctx, p, eh, ec, n_procs, host=False):
    E, total = len(eh), int(np.sum(n_procs))
    d, a = np.zeros(max(E, 1), np.int64), np.zeros(max(total, 1), _lib.PROC_ATTR_DTYPE)
    rp, pp = p.params(), p.procset_params()
    L = _lib.load()
    eh, ec, n_procs = (np.ascontiguousarray(eh, np.uint64), np.ascontiguousarray(ec, np.uint8),
                       np.ascontiguousarray(n_procs, np.uint32))
    if host:
        rc = L.nmz_procset_decide_host(int(p.Seed), _lib.ptr(eh), _lib.ptr(ec), _lib.ptr(n_procs), E,
                                       ctypes.byref(rp), ctypes.byref(pp), _lib.ptr(d), _lib.ptr(a))
    else:
        rc = L.nmz_procset_decide(ctx.handle, int(p.Seed), _lib.ptr(eh), _lib.ptr(ec), _lib.ptr(n_procs), E,
                                  ctypes.byref(rp), ctypes.byref(pp), _lib.ptr(d), _lib.ptr(a))
    return d[:E], a[:total], rc


@pytest.mark.parametrize("name", POLICIES)
def test_wide_interval(ctx, name):
    """(0, 2^62 + 1): about half of the delay draws are rejected, so about half of the lanes of every wave leave
    the uniform path on every event. 512 seeds x 4 events x 24 processes."""
    p, rp, ref = policy(name, interval=WIDE)
    eh = RNG.integers(0, 2**64, size=4, dtype=np.uint64)
    ec = np.array([0, 1, 0, 1], np.uint8)
    n_procs = np.full(4, 24, np.uint32)
    target = np.array([0, 23, NONE, 11], np.uint32)
    st, dl, at, outs = R.sweep(5, 512, eh, ec, n_procs, target, rp, ref, n_dump=3)
    redrawn = []
    for i in range(512):  # the delay draw alone, with the oracle's generator
        g = O.GoRand(O.random_event_seed(5 + i, int(eh[0])))
        g.int63n(WIDE[1] - WIDE[0])
        redrawn.append(g.n_out > 1)
    assert 0.3 < np.mean(redrawn) < 0.7
    r = p.ProcSetSweep(5, 512, eh, ec, n_procs, target, n_dump=3, k=8, ctx=ctx)
    assert same_stats(r.stats, st) and np.array_equal(r.delays, dl) and same_attrs(r.attrs, at)
    assert same_topk(r.topk, R.topk(st, 5, 8, True))


@pytest.mark.parametrize("name", POLICIES)
def test_cross_path_equality(ctx, name):
    """nmz_procset_decide == nmz_procset_decide_host == the sweep's dump row, for the same seed (and the reference)."""
    p, rp, ref = policy(name, prioritized=64, seed=SEED0 + 2)
    n_procs, target = sweep_case(name)
    d1, a1, rc1 = _decide(ctx, p, EVHASH, EVCLASS, n_procs)
    d2, a2, rc2 = _decide(ctx, p, EVHASH, EVCLASS, n_procs, host=True)
    assert rc1 == rc2 == 0
    r = p.ProcSetSweep(SEED0, 3, EVHASH, EVCLASS, n_procs, target, n_dump=3, ctx=ctx)
    assert np.array_equal(d1, d2) and np.array_equal(a1, a2)
    assert np.array_equal(d1, r.delays[2]) and np.array_equal(a1, r.attrs[2])
    dl, at = R.decide_events(p.Seed, EVHASH, EVCLASS, n_procs, rp, ref)
    assert np.array_equal(d1, dl) and same_attrs(a1, at)
    # and the statistics of the same call: the sweep kernel's uniform form at prioritized = 64
    st, _, _, _ = R.sweep(SEED0, 3, EVHASH, EVCLASS, n_procs, target, rp, ref)
    assert same_stats(r.stats, st)


def test_edge_cases(ctx):
    p, rp, ref = policy("mild")
    # zero events: zeroed stats with flags = 0, the smallest seeds first
    r = p.ProcSetSweep(3, 5, np.zeros(0, np.uint64), np.zeros(0, np.uint8), np.zeros(0, np.uint32), k=3, ctx=ctx)
    assert r.stats.tobytes() == bytes(5 * 32)
    assert r.topk["seed"].tolist() == [3, 4, 5] and r.topk["target_score"].tolist() == [0, 0, 0]
    # a seed range wrapping past 2^64, and k larger than the number of seeds
    eh = RNG.integers(0, 2**64, size=20, dtype=np.uint64)
    ec = RNG.integers(0, 2, size=20, dtype=np.uint8)
    n_procs = RNG.integers(0, 30, size=20).astype(np.uint32)
    target = np.where(n_procs > 0, 0, NONE).astype(np.uint32)
    st, dl, at, _ = R.sweep(2**64 - 3, 7, eh, ec, n_procs, target, rp, ref, n_dump=7)
    r = p.ProcSetSweep(2**64 - 3, 7, eh, ec, n_procs, target, n_dump=7, k=9, descending=False, ctx=ctx)
    assert same_stats(r.stats, st) and np.array_equal(r.delays, dl) and same_attrs(r.attrs, at)
    assert same_topk(r.topk, R.topk(st, 2**64 - 3, 9, False))
    assert r.topk["seed"][7:].tolist() == [2**64 - 1] * 2 and r.topk["target_score"][7:].tolist() == [-2**63] * 2
    # k = 256
    st, _, _, _ = R.sweep(100, 700, eh[:3], ec[:3], n_procs[:3], target[:3], rp, ref)
    r = p.ProcSetSweep(100, 700, eh[:3], ec[:3], n_procs[:3], target[:3], k=256, ctx=ctx)
    assert same_stats(r.stats, st) and same_topk(r.topk, R.topk(st, 100, 256, True))
    with pytest.raises(_lib.NmzInvalidArgument):
        p.ProcSetSweep(100, 700, eh[:3], ec[:3], n_procs[:3], k=257, ctx=ctx)


@pytest.mark.parametrize("name,n,kw,match", [
    ("mild", 513, {}, "n_procs exceeds 512"),
    ("extreme", 0, {"prioritized": 1}, "no process"),
    ("dirichlet", 0, {}, "has no process"),
])
def test_invalid_arguments_on_the_device_entry_points(ctx, name, n, kw, match):
    p, _, _ = policy(name, **kw)
    eh, ec, n_procs = np.array([1, 2], np.uint64), np.zeros(2, np.uint8), np.array([4, n], np.uint32)
    with pytest.raises(_lib.NmzInvalidArgument, match=match):
        p.ProcSetSweep(0, 5, eh, ec, n_procs, ctx=ctx)
    assert _decide(ctx, p, eh, ec, n_procs)[2] == _lib.NMZ_EINVAL


def test_invalid_class_bits_and_params(ctx):
    p, _, _ = policy("mild")
    eh, n_procs = np.array([1, 2], np.uint64), np.array([4, 4], np.uint32)
    for bits in (_lib.NMZ_EV_FAULTABLE, 4):
        ec = np.array([0, bits], np.uint8)
        with pytest.raises(_lib.NmzInvalidArgument, match="NMZ_EV_PRIORITIZED only"):
            p.ProcSetSweep(0, 5, eh, ec, n_procs, ctx=ctx)
        assert _decide(ctx, p, eh, ec, n_procs)[2] == _lib.NMZ_EINVAL
    with pytest.raises(_lib.NmzInvalidArgument, match="target_slot"):
        p.ProcSetSweep(0, 5, eh, np.zeros(2, np.uint8), n_procs, np.array([4, 0], np.uint32), ctx=ctx)
    # prioritized 257 passed straight to the entry point (the resolver refuses it first)
    pp = _lib.ProcSetParams(_lib.NMZ_PROC_EXTREME, 1, 257, 0)
    rp = p.params()
    ec = np.zeros(2, np.uint8)
    st = np.zeros(5, _lib.PROCSET_STATS_DTYPE)
    rc = _lib.load().nmz_procset_sweep(ctx.handle, 0, 5, _lib.ptr(eh), _lib.ptr(ec), _lib.ptr(n_procs), None, 2,
                                       ctypes.byref(rp), ctypes.byref(pp), _lib.ptr(st), None, None, 0, 0, 1, None)
    assert rc == _lib.NMZ_EINVAL and "prioritized exceeds 256" in _lib.last_error()
    # the K2 sweep still refuses the class bit it never knew
    with pytest.raises(_lib.NmzInvalidArgument, match="unknown bits"):
        p.Sweep(0, 5, np.zeros(2, np.uint64), np.array([4, 0], np.uint8), ctx=ctx)
