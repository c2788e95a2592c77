"""GPU parity of the wavelet-tree sweep's top-k from per-chunk maxima (k_replayable_sweep_wt's chunk records and
k_wt_topk_chunks): every case sweeps through the C ABI and asserts that the stats equal the oracle's bit for bit and
that the top-k equals the oracle's top-k of those stats. Small traces (30-300 events); the cases sit where the
selection changes path: the chunk count around k, chunk edges, ties at the threshold, the candidate and flagged-chunk
overflows, records left by a larger sweep, wrapping seeds, the BIG kernel form and the NMZ_WT_G knob."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from namazu_amd import _lib
from namazu_amd.explorepolicy import to_csr
from oracle import oracle as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WT_CAND = 4096  # csrc/replayable_wt_dev.h: the candidate arrays (and the list of flagged chunks)


def zk_hints(n, seed):
    v = np.random.default_rng(seed).integers(-2**63, 2**63 - 1, size=n, dtype=np.int64)
    return [str(int(x)) for x in v]


def rep_oracle(seeds, hints, m):
    so, sb = O.to_csr(seeds)
    ho, hb = O.to_csr(hints)
    return O.replayable_sweep(so, sb, ho, hb, m, n_dump=0)[0]


_POOL = {}


def row_pool():
    """Decimal strings 0 .. 149,999 by the low byte of their FNV-1a 64 (the table row, i.e. the bucket of the sweep):
    ~580 strings per row."""
    if not _POOL:
        off, prime = np.uint64(0xCBF29CE484222325), np.uint64(0x100000001B3)
        strs = np.arange(0, 150_000).astype(str)
        lens = np.char.str_len(strs)
        h = np.zeros(len(strs), np.uint64)
        for ln in np.unique(lens):
            sel = lens == ln
            b = np.frombuffer("".join(strs[sel]).encode(), np.uint8).reshape(-1, ln)
            x = np.full(b.shape[0], off, np.uint64)
            with np.errstate(over="ignore"):
                for k in range(ln):
                    x = (x ^ b[:, k].astype(np.uint64)) * prime
            h[sel] = x
        rows = (h & np.uint64(0xFF)).astype(np.int64)
        for r in range(256):
            _POOL[r] = [str(s) for s in strs[rows == r]]
    return _POOL


def seeds_by_rows(counts, shuffle_seed=1):
    """counts: {row: n} -> n distinct seed strings in each of the rows, in a shuffled order"""
    pool = row_pool()
    out = []
    for row, n in counts.items():
        assert n <= len(pool[row])
        out += pool[row][:n]
    rng = np.random.default_rng(shuffle_seed)
    return [out[i] for i in rng.permutation(len(out))]


def n_chunks(seeds):
    """chunks of 64 seeds per row, as the sweep forms them"""
    rows = np.zeros(256, np.int64)
    for s in seeds:
        h = 0xCBF29CE484222325
        for c in s.encode():
            h = ((h ^ c) * 0x100000001B3) & (2**64 - 1)
        rows[h & 0xFF] += 1
    return int(((rows + 63) // 64).sum())


class Plan:
    def __init__(self, ctx, hints, m, max_seeds):
        self.L = _lib.load()
        ho, hb = to_csr(hints)
        self.h = ctypes.c_void_p()
        _lib.check(self.L.nmz_replayable_plan_create(ctx.handle, _lib.ptr(ho), _lib.ptr(hb), len(hints), m, max_seeds,
                                                     ctypes.byref(self.h)))

    def _run(self, S, k, call):
        import torch
        d_st = torch.zeros(S * 32, dtype=torch.uint8, device="cuda")
        d_tk = torch.zeros(k * 24, dtype=torch.uint8, device="cuda")
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        _lib.check(call(ctypes.c_void_p(d_st.data_ptr()), ctypes.c_void_p(d_tk.data_ptr()), stream))
        torch.cuda.synchronize()
        st = np.frombuffer(d_st.cpu().numpy().tobytes(), dtype=_lib.SCHED_STATS_DTYPE)
        tk = np.frombuffer(d_tk.cpu().numpy().tobytes(), dtype=_lib.TOPK_DTYPE)
        return st, tk

    def csr(self, seeds, seed0, k):
        import torch
        so, sb = to_csr(seeds)
        d_so = torch.from_numpy(so.view(np.int32)).cuda()
        d_sb = torch.from_numpy(sb).cuda()
        return self._run(len(seeds), k, lambda st, tk, s: self.L.nmz_replayable_sweep_topk_dev(
            self.h, ctypes.c_void_p(d_so.data_ptr()), ctypes.c_void_p(d_sb.data_ptr()), len(seeds), seed0, k, st, tk,
            s))

    def decimal(self, lo, S, k):
        return self._run(S, k, lambda st, tk, s: self.L.nmz_replayable_sweep_decimal_topk_dev(self.h, lo, S, k, st,
                                                                                            tk, s))

    def close(self):
        self.L.nmz_replayable_plan_destroy(self.h)


def check_csr(ctx, seeds, hints, m, k, seed0=0):
    """one CSR sweep on its own plan: stats == the oracle's, top-k == the oracle's top-k of them; returns both"""
    p = Plan(ctx, hints, m, len(seeds))
    try:
        st, tk = p.csr(seeds, seed0, k)
    finally:
        p.close()
    ost = rep_oracle(seeds, hints, m)
    assert st.tobytes() == ost.tobytes()
    exp = O.topk_from_stats(ost, seed0, k)
    assert tk.tolist() == exp.tolist()
    return ost, exp


@pytest.mark.parametrize("rows,chunks", [({3: 70, 200: 10}, 3), ({3: 70, 200: 10, 77: 1}, 4),
                                         ({3: 130, 200: 64, 77: 1}, 5)])
def test_chunk_count_around_k(ctx, rows, chunks):
    """k = 4 with 3, 4 and 5 chunks: fewer chunks than k (tau 0, every seed a candidate), as many (tau the smallest
    chunk maximum), one more (the first real selection)."""
    seeds = seeds_by_rows(rows)
    assert n_chunks(seeds) == chunks
    check_csr(ctx, seeds, zk_hints(120, 5), 100_000_000, 4)


def test_chunk_edges(ctx):
    """Rows of exactly 64, 65 and 128 seeds (one full chunk; a full one and one seed; two full), rows of one seed,
    every other row empty."""
    rows = {0: 64, 9: 65, 255: 128, 1: 1, 100: 1, 254: 1, 31: 1}
    seeds = seeds_by_rows(rows, 2)
    assert n_chunks(seeds) == 1 + 2 + 2 + 4
    for k in (16, 64):
        check_csr(ctx, seeds, zk_hints(200, 6), 100_000_000, k)


def test_one_seed(ctx):
    """S = 1: one chunk of one seed, then sentinels."""
    _, exp = check_csr(ctx, ["foobar"], zk_hints(30, 7), 1_000_000_000, 4)
    assert int(exp["seed"][0]) == 0 and int(exp["seed"][1]) == 2**64 - 1


def test_tau_is_a_bound_not_the_kth_seed(ctx):
    """The best seed string 100 times among 5,000 others, k = 64: the copies fill two or three chunks of their row, so
    tau (the 64th largest chunk maximum) lies well below them and the candidates hold far more than 64 seeds; the
    answer is the 64 lowest indices of the copies."""
    hints, m = zk_hints(100, 8), 100_000_000
    others = [str(i * 7919 + 13) for i in range(5000)]
    ost = rep_oracle(others, hints, m)
    best = others[int(np.argmax(ost["sum_delay_ns"].astype(np.int64)))]
    rng = np.random.default_rng(9)
    seeds = list(others)
    for pos in sorted(rng.integers(0, 5000, 100).tolist(), reverse=True):
        seeds.insert(pos, best)
    copies = [i for i, s in enumerate(seeds) if s == best]
    assert len(copies) == 101
    _, exp = check_csr(ctx, seeds, hints, m, 64)
    assert exp["seed"].tolist() == copies[:64]


@pytest.mark.parametrize("m,S,k", [(7, 6000, 33), (1, 4096, 5)])
def test_ties_at_tau(ctx, m, S, k):
    """maxInterval 7: sums of 0..6 per event, many chunks share the largest maximum and the seeds at tau overflow the
    candidate arrays (the exact selection). maxInterval 1: every sum 0, every chunk flagged and exactly WT_CAND
    candidates (two full sort chunks)."""
    assert S != 4096 or S == WT_CAND
    check_csr(ctx, [str(i * 7919) for i in range(S)], zk_hints(100, 10), m, k, seed0=3)


def test_tied_candidates_of_few_full_chunks(ctx):
    """maxInterval 1 over 40 rows of exactly 64 seeds: 40 flagged chunks are read in one round, and their 2,560 tied
    candidates need two sort chunks (between one chunk's 2,048 and WT_CAND)."""
    seeds = seeds_by_rows({r: 64 for r in range(100, 140)}, 3)
    assert n_chunks(seeds) == 40
    check_csr(ctx, seeds, zk_hints(40, 14), 1, 5, seed0=2**64 - 100)


def test_more_flagged_chunks_than_candidates(ctx):
    """maxInterval 1 over 300,000 decimal seeds: ~4,700 chunks, all at tau = the one key, more than WT_CAND of them:
    the direct exact selection over the stats in seed order. The answer is the five lowest seeds."""
    lo, S, k, hints = 1000, 300_000, 5, zk_hints(30, 11)
    assert S // 64 > WT_CAND
    p = Plan(ctx, hints, 1, S)
    try:
        st, tk = p.decimal(lo, S, k)
    finally:
        p.close()
    ost = rep_oracle([str(lo + i) for i in range(S)], hints, 1)
    assert st.tobytes() == ost.tobytes()
    exp = O.topk_from_stats(ost, lo, k)
    assert exp["seed"].tolist() == [lo + i for i in range(k)]
    assert tk.tolist() == exp.tolist()


def test_stale_records_of_a_larger_sweep(ctx):
    """One plan sweeps 9,000 seeds and then 3,000 others: the second selection reads only its own sweep's chunk
    records (the first left ~3x as many in the same scratch)."""
    hints, m, k = zk_hints(150, 12), 100_000_000, 64
    a = [str(i * 7919) for i in range(9000)]
    b = [str(10**9 + i * 104_729) for i in range(3000)]
    p = Plan(ctx, hints, m, len(a))
    try:
        got = [p.csr(s, 0, k) for s in (a, b)]
    finally:
        p.close()
    for seeds, (st, tk) in zip((a, b), got):
        ost = rep_oracle(seeds, hints, m)
        assert st.tobytes() == ost.tobytes()
        assert tk.tolist() == O.topk_from_stats(ost, 0, k).tolist()


@pytest.mark.parametrize("m,S,k,seed0", [(100_000_000, 5000, 64, 2**64 - 1500),  # seeds wrap past 2^64
                                         (100_000_000, 5000, 1, 0),                # k = 1
                                         (2**31 + 3, 4000, 16, 2**64 - 1500),     # m >= 2^31: the BIG kernel form
                                         (2**32 - 1, 2500, 1, 7),
                                         (2**32 - 1, 6000, 64, 0)])  # chunk maxima spread over more than 32 bits
def test_seed_wrap_k1_and_big_moduli(ctx, m, S, k, seed0):
    check_csr(ctx, [str(i * 7919 + 1) for i in range(S)], zk_hints(60, 13), m, k, seed0=seed0)


def _child_case():
    """run in a fresh process (NMZ_WT_G is read once per process): two workgroups per row share a row's chunks"""
    ctx = _lib.Context(0)
    try:
        seeds = seeds_by_rows({3: 130, 200: 64, 77: 1, 5: 300, 6: 65})
        check_csr(ctx, seeds, zk_hints(120, 5), 100_000_000, 4)
        check_csr(ctx, [str(i * 7919) for i in range(6000)], zk_hints(100, 10), 100_000_000, 64, seed0=2**64 - 1500)
    finally:
        ctx.close()
    print("child ok")


def test_two_workgroups_per_row_in_a_fresh_process():
    """NMZ_AB=1 NMZ_WT_G=2: a chunk's record slot depends on (row, chunk) alone, whichever workgroup takes it."""
    env = {k: v for k, v in os.environ.items() if not k.startswith("NMZ_")}
    env.update(NMZ_AB="1", NMZ_WT_G="2")
    code = ("import sys; sys.path[:0] = [%r, %r]; import test_wt_topk_chunks_gpu as t; t._child_case()"
            % (ROOT, os.path.join(ROOT, "tests")))
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "child ok" in r.stdout, r.stdout + r.stderr
