"""CPU: the Go-seed reduction of the random policy's sweeps at its edges. go_seed_from_table
(namazu_amd/csrc/random_dev.h) reduces int64(FNV1a64(le64(seed) || le64(evhash))) mod 2^31 - 1 from residues with four
data-dependent corrections that fire about once in 2^31 decisions each; tests/golden/go_seed_edges.json holds
searched vectors (tools/find_go_seed_edges.c) that take every one of them. Here: the fixture is what it claims to be
and covers every class, the restated arithmetic (tests/go_seed_ref.py) equals x mod M31, and the host decision paths
(the seed_reduce direct form) decide the vectors as the oracle does. The kernels run them in
tests/test_go_seed_edges_gpu.py."""
import ctypes
import itertools

import numpy as np
import pytest

import go_seed_ref as G
import procset_ref as R
from namazu_amd import _lib
from oracle import oracle as O

M31 = G.M31
INTERVALS = [(30_000_000, 100_000_000), (0, 3_000_000_000), (5_000_000, 5_000_000), (0, 2**62 + 1)]


@pytest.fixture(scope="module")
def vectors(golden):
    return golden("go_seed_edges.json")["vectors"]


def test_fixture_vectors_are_what_they_record(vectors):
    """Per vector: the decomposition's seed == Go's rule over the oracle's hash == the recorded go_seed, every
    recorded label is reproduced, and the class's definition holds."""
    assert 0 < len(vectors) <= 40
    for v in vectors:
        seed, eh = v["seed"], v["evhash"]
        u, H, C = G.decompose(seed, eh)
        assert (H + C) & G.M64 == u
        assert u == O.random_event_seed(seed, eh) & G.M64
        s, k, carry, sign, s1, folded, borrowed, zero = G.table_seed(seed, eh)
        assert s == G.direct_seed(seed, eh) == v["go_seed"], v
        assert (k, carry, sign, s1) == (v["k"], v["carry"], v["sign"], v["s1"]), v
        t = s1 - M31 if folded else s1
        assert t == v["t"] and folded == (v["s1"] >= M31), v
        spec = G.CLASSES[v["class"]]
        assert k == spec["k"] and s == spec["go_seed"], v
        assert s1 == spec["s1"] if "s1" in spec else t == spec["t"], v
        assert borrowed == (t < 4 * k) and zero == (s == G.ZERO_SEED), v
        assert 2048 <= seed < 2**32  # seed - 2048 does not wrap


def test_fixture_covers_every_class(vectors):
    """Every class of tools/find_go_seed_edges.c has a vector: none may be missing."""
    have = {v["class"] for v in vectors}
    assert sorted(set(G.CLASSES) - have) == [] and have <= set(G.CLASSES)
    k1 = [(v["carry"], v["sign"]) for v in vectors if v["k"] == 1]
    assert (1, 0) in k1 and (0, 1) in k1  # the wrap alone and the sign alone
    assert any(v["carry"] == v["sign"] == 1 for v in vectors if v["k"] == 2)
    t_folded = {v["s1"] >= M31 for v in vectors if "_t" in v["class"]}
    assert t_folded == {True, False}
    # H < 2^63 reaches k in {0, 1}, H >= 2^63 reaches k in {1, 2}: at least one policy seed of each kind
    high = {v["seed"]: G.decompose(v["seed"], 0)[1] >> 63 for v in vectors}
    assert set(high.values()) == {0, 1}
    for v in vectors:
        assert v["k"] in ((1, 2) if high[v["seed"]] else (0, 1))
    # all four corrections and both extreme seeds are present
    flags = [G.table_seed(v["seed"], v["evhash"])[5:] for v in vectors]
    assert {f[0] for f in flags} == {f[1] for f in flags} == {f[2] for f in flags} == {True, False}
    assert {1, M31 - 1, G.ZERO_SEED} <= {v["go_seed"] for v in vectors}


def expected_mod(hm, cm, k):
    x = (hm + cm - 4 * k) % M31
    return G.ZERO_SEED if x == 0 else x


def test_restated_arithmetic_is_mod_m31():
    """residues() against x mod M31: every pair of the edge residues with k = 0, 1, 2; 10^5 random triples; and
    the whole decomposition against Go's rule for random 64-bit (H, C)."""
    edge = [0, 1, 2, 7, 8, 9] + list(range(M31 - 9, M31))
    n = 0
    for hm, cm, k in itertools.product(edge, edge, (0, 1, 2)):
        assert G.residues(hm, cm, k)[0] == expected_mod(hm, cm, k), (hm, cm, k)
        n += 1
    assert n == 15 * 15 * 3
    rng = np.random.default_rng(31)
    hms, cms = rng.integers(0, M31, size=(2, 100_000)).tolist()
    for hm, cm, k in zip(hms, cms, rng.integers(0, 3, size=100_000).tolist()):
        assert G.residues(hm, cm, k)[0] == expected_mod(hm, cm, k), (hm, cm, k)
    for H, C in rng.integers(0, 2**64, size=(20_000, 2), dtype=np.uint64).tolist():
        u = (H + C) & G.M64
        k = ((H + C) >> 64) + (u >> 63)
        assert G.residues(H % M31, C % M31, k)[0] == G.go_reduce(u - (1 << 64) if u >> 63 else u), (H, C)


def test_go_reduce_is_gos_rule():
    for x, s in [(0, G.ZERO_SEED), (M31, G.ZERO_SEED), (-M31, G.ZERO_SEED), (1, 1), (-1, M31 - 1), (M31 + 1, 1),
                 (-(1 << 63), M31 - 2), ((1 << 63) - 1, 1), (-(1 << 63) + 2, G.ZERO_SEED)]:
        assert G.go_reduce(x) == s, x


def by_seed(vectors):
    return {s: [v["evhash"] for v in vectors if v["seed"] == s] for s in sorted({v["seed"] for v in vectors})}


@pytest.mark.parametrize("mn,mx", INTERVALS)
def test_random_decide_host_on_the_vectors(vectors, mn, mx):
    """nmz_random_decide_host (gorand::seed_reduce, then decide() entered with s = 1, M31 - 1, 89482311, ...) vs
    the oracle's full rand.Seed per decision: every vector, every event class, p = 0.1 and 0.9."""
    L = _lib.load()
    for (seed, hashes), p in itertools.product(by_seed(vectors).items(), (0.1, 0.9)):
        eh = np.repeat(np.array(hashes, np.uint64), 4)
        ec = np.tile(np.arange(4, dtype=np.uint8), len(hashes))
        d, f = np.zeros(len(eh), np.int64), np.zeros(len(eh), np.uint8)
        params, pr = _lib.resolve_random_params(mn, mx, p), O.random_params(mn, mx, p)
        _lib.check(L.nmz_random_decide_host(seed, _lib.ptr(eh), _lib.ptr(ec), len(eh), ctypes.byref(params),
                                            _lib.ptr(d), _lib.ptr(f)))
        for i in range(len(eh)):
            od, of, _ = O.random_decide(seed, int(eh[i]), int(ec[i]), pr)
            assert (int(d[i]), bool(f[i])) == (od, of), (seed, int(eh[i]), int(ec[i]), p)


@pytest.mark.parametrize("name", ["mild", "extreme", "dirichlet"])
@pytest.mark.parametrize("mn,mx", INTERVALS)
def test_procset_decide_host_on_the_vectors(vectors, name, mn, mx):
    """nmz_procset_decide_host on every vector as a ProcSetEvent (5 processes, one event with 410; both entity
    classes) vs the plain-Python reference."""
    L = _lib.load()
    pol = ["mild", "extreme", "dirichlet"].index(name)
    ref, pp = R.Params(pol, True, 3, 0.1), _lib.resolve_procset_params(name, True, 3, 0.1)
    params, pr = _lib.resolve_random_params(mn, mx, 0.1), O.random_params(mn, mx, 0.1)
    for seed, hashes in by_seed(vectors).items():
        eh = np.repeat(np.array(hashes, np.uint64), 2)
        ec = np.tile(np.arange(2, dtype=np.uint8), len(hashes))
        n_procs = np.full(len(eh), 5, np.uint32)
        n_procs[1] = 410
        d, a = np.zeros(len(eh), np.int64), np.zeros(int(n_procs.sum()), _lib.PROC_ATTR_DTYPE)
        rc = L.nmz_procset_decide_host(seed, _lib.ptr(eh), _lib.ptr(ec), _lib.ptr(n_procs), len(eh),
                                       ctypes.byref(params), ctypes.byref(pp), _lib.ptr(d), _lib.ptr(a))
        rd, ra = R.decide_events(seed, eh, ec, n_procs, pr, ref)
        assert rc == 0 and np.array_equal(d, rd) and np.array_equal(a.astype(R.ATTR_DTYPE), ra), seed
