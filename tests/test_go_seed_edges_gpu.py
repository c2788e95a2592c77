"""GPU: the Go-seed reduction of the random policy's sweeps at its edges. Both instantiations of k_random_sweep and
k_procset_sweep reduce the per-decision seed with go_seed_from_table (csrc/random_dev.h): a fold at s1 >= M31, a
borrow when 4k exceeds the folded value, and the zero map, each taken about once in 2^31 decisions, so no random
input reaches them. The vectors of tests/golden/go_seed_edges.json (tools/find_go_seed_edges.c; checked on the CPU
by tests/test_go_seed_edges.py) take every one of them, and end in the extreme Go seeds 1, M31 - 1 and 89482311.
Everything is integer: every comparison is equality against the oracle (tests/procset_ref.py for ProcSetEvents)."""
import ctypes

import numpy as np
import pytest

import go_seed_ref as G
import procset_ref as R
from namazu_amd import _lib
from namazu_amd.explorepolicy import Random
from oracle import oracle as O

pytestmark = pytest.mark.gpu

SEEDS = [2581, 7153, 735232460]  # the fixture's policy seeds: H < 2^63, H >= 2^63, Hm = 0 (unfolded t classes)
INTERVALS = {"k32": (30_000_000, 100_000_000),  # k_random_sweep<true>
             "general": (0, 3_000_000_000),     # k_random_sweep<false>
             "fixed": (5_000_000, 5_000_000),   # no delay draw: the fault draw alone
             "wide": (0, 2**62 + 1)}            # about half of the delay draws rejected: go_output from edge seeds
POLICIES = ["mild", "extreme", "dirichlet"]
NONE = _lib.NMZ_NONE


def seed_vectors(golden, seed):
    """The seed's vectors, after checking that they are still what the fixture records: a stale fixture must fail
    rather than test nothing."""
    g = golden("go_seed_edges.json")["vectors"]
    assert sorted({v["seed"] for v in g}) == SEEDS
    assert {v["class"] for v in g} == set(G.CLASSES)
    vs = [v for v in g if v["seed"] == seed]
    for v in vs:
        assert G.go_reduce(O.random_event_seed(seed, v["evhash"])) == v["go_seed"], v
    assert {1, G.M31 - 1, G.ZERO_SEED} <= {v["go_seed"] for v in vs}
    return vs


def k2_events(golden, seed):
    """The vectors twice (the second copy prioritized) between random filler hashes, all faultable."""
    hits = np.array([v["evhash"] for v in seed_vectors(golden, seed)], np.uint64)
    fill = np.random.default_rng(seed).integers(0, 2**64, size=23, dtype=np.uint64)
    eh = np.concatenate([fill[:7], hits, fill[7:15], hits, fill[15:]])
    ec = np.full(len(eh), _lib.NMZ_EV_FAULTABLE, np.uint8)
    ec[7 + len(hits) + 8:7 + 2 * len(hits) + 8] |= _lib.NMZ_EV_PRIORITIZED
    return eh, ec


def random_policy(mn, mx, p, seed=0):
    rp = Random()
    rp.MinInterval, rp.MaxInterval, rp.FaultActionProbability, rp.Seed = mn, mx, p, seed
    return rp


@pytest.mark.parametrize("before,n", [(100, 201), (2048, 4096)])  # 4,096: ~16 seeds of the vector seed's bucket
@pytest.mark.parametrize("p", [0.1, 0.9])                         # share its wave, so it is not always lane 0
@pytest.mark.parametrize("kind", list(INTERVALS))
@pytest.mark.parametrize("seed", SEEDS)
def test_random_sweep_on_the_vectors(ctx, golden, seed, kind, p, before, n):
    """The statistics path alone (no dump, which goes through seed_reduce): stats and top-8 of every seed around
    the vectors' seed."""
    mn, mx = INTERVALS[kind]
    eh, ec = k2_events(golden, seed)
    seed0 = seed - before
    r = random_policy(mn, mx, p).Sweep(seed0, n, eh, ec, k=8, ctx=ctx)
    st, _, _ = O.random_sweep(seed0, n, eh, ec, O.random_params(mn, mx, p))
    assert np.array_equal(r.stats[before], st[before])  # the vectors' seed first, for a readable failure
    assert np.array_equal(r.stats, st)
    assert np.array_equal(r.topk, O.topk_from_stats(st, seed0, 8))


@pytest.mark.parametrize("p", [0.1, 0.9])
@pytest.mark.parametrize("kind", list(INTERVALS))
@pytest.mark.parametrize("seed", SEEDS)
def test_random_dump_and_online_on_the_vectors(ctx, golden, seed, kind, p):
    """The same events with the vectors' seed among the dumped ones (k_random_dump), and through nmz_random_decide
    (k_random_decide): the seed_reduce direct form, per decision against the oracle."""
    mn, mx = INTERVALS[kind]
    eh, ec = k2_events(golden, seed)
    pr = O.random_params(mn, mx, p)
    rp = random_policy(mn, mx, p, seed)
    r = rp.Sweep(seed - 3, 8, eh, ec, n_dump=8, ctx=ctx)
    st, dl, fl = O.random_sweep(seed - 3, 8, eh, ec, pr, n_dump=8)
    assert np.array_equal(r.delays, dl) and np.array_equal(r.faults, fl) and np.array_equal(r.stats, st)
    d, f = np.zeros(len(eh), np.int64), np.zeros(len(eh), np.uint8)
    params = rp.params()
    _lib.check(_lib.load().nmz_random_decide(ctx.handle, seed, _lib.ptr(eh), _lib.ptr(ec), len(eh),
                                             ctypes.byref(params), _lib.ptr(d), _lib.ptr(f)))
    exp = [O.random_decide(seed, int(h), int(c), pr)[:2] for h, c in zip(eh, ec)]
    assert d.tolist() == [e[0] for e in exp] and f.astype(bool).tolist() == [e[1] for e in exp]
    assert np.array_equal(d, dl[3]) and np.array_equal(f, fl[3])


@pytest.mark.parametrize("kind", ["k32", "fixed", "wide"])
@pytest.mark.parametrize("name", POLICIES)
@pytest.mark.parametrize("seed", SEEDS)
def test_procset_on_the_vectors(ctx, golden, seed, name, kind):
    """The vectors as ProcSetEvents: k_procset_sweep is the second, separately compiled use of go_seed_from_table
    (with its default arguments). 5 processes per vector event, one with 410; the statistics path (no dump), then
    nmz_procset_decide for the vectors' seed."""
    mn, mx = INTERVALS[kind]
    p = random_policy(mn, mx, 0.0, seed)
    p.ProcPolicy = name
    p.PPPMild.UseBatch, p.PPPExtreme.Prioritized, p.PPPDirichlet.ResetProbability = True, 3, 0.1
    rp, ref = O.random_params(mn, mx, 0.0), R.Params(POLICIES.index(name), True, 3, 0.1)
    hh = np.array([v["evhash"] for v in seed_vectors(golden, seed)], np.uint64)
    hn = [5] * len(hh)
    hn[len(hh) // 2] = 410
    fill = np.random.default_rng(seed + 1).integers(0, 2**64, size=9, dtype=np.uint64)
    eh = np.concatenate([fill[:3], hh, fill[3:6], hh, fill[6:]])
    n_procs = np.array([3, 17, 1] + hn + [8, 5, 2] + [5] * len(hh) + [4, 33, 6], np.uint32)
    ec = np.zeros(len(eh), np.uint8)
    ec[3 + len(hh) + 3:3 + 2 * len(hh) + 3] = _lib.NMZ_EV_PRIORITIZED
    target = np.where(np.arange(len(eh)) % 2 == 0, n_procs - 1, NONE).astype(np.uint32)
    seed0 = seed - 100
    st, _, _, _ = R.sweep(seed0, 201, eh, ec, n_procs, target, rp, ref)
    r = p.ProcSetSweep(seed0, 201, eh, ec, n_procs, target, k=8, ctx=ctx)
    got = np.asarray(r.stats).astype(R.STATS_DTYPE)
    assert np.array_equal(got[100], st[100])
    assert np.array_equal(got, st)
    assert np.array_equal(np.asarray(r.topk).astype(R.TOPK_DTYPE), R.topk(st, seed0, 8, True))
    d, a = np.zeros(len(eh), np.int64), np.zeros(int(n_procs.sum()), _lib.PROC_ATTR_DTYPE)
    params, pp = p.params(), p.procset_params()
    _lib.check(_lib.load().nmz_procset_decide(ctx.handle, seed, _lib.ptr(eh), _lib.ptr(ec), _lib.ptr(n_procs),
                                              len(eh), ctypes.byref(params), ctypes.byref(pp), _lib.ptr(d),
                                              _lib.ptr(a)))
    dl, at = R.decide_events(seed, eh, ec, n_procs, rp, ref)
    assert np.array_equal(d, dl) and np.array_equal(a.astype(R.ATTR_DTYPE), at)
