"""ProcSet sweep rate (a tool, not a bench leg): 2^20 seeds x 1,000 ProcSetEvents x 32 processes per policy.

For each of mild, extreme and dirichlet: three repetitions of 5 warm-up sweeps and then 20 timed sweeps through
nmz_procset_sweep (each call ends in a stream synchronise); the time is the sweep kernel's, from device events
around its launch (nmz_timing_enable / nmz_timing_read "procset_sweep"). Reports process-decisions/s, generator
outputs/s (every decision's outputs, counted from the statistics of one sweep: 1 delay draw + the sub-policy's
draws) and the spread over the repetitions, and writes the record as JSON.
usage: python3 tools/procset_rate.py [--seeds N] [--events E] [--procs P] [--timed 20]
                                     [--out profiles/procset/rate.json]
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
from namazu_amd import _lib  # noqa: E402
from namazu_amd.explorepolicy import Random  # noqa: E402


def splitmix64(seed, n):
    """n event hashes: SplitMix64 of seed, seed + 1, ..."""
    z = (np.arange(n, dtype=np.uint64) + np.uint64(seed)) + np.uint64(0x9E3779B97F4A7C15)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


# K2's rate for context, from its committed profile (profiles/r06am_random_kernel_stats.csv): k_random_sweep takes
# 247.5 ms for 10^7 seeds x 10^4 events, two generator outputs per decision (delay + fault draw)
K2_CONTEXT = {"source": "profiles/r06am_random_kernel_stats.csv", "kernel_ms": 247.498, "decisions": 1e11,
              "outputs_per_decision": 2, "outputs_per_s": 2e11 / 0.247498}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", type=int, default=1 << 20)
    ap.add_argument("--events", type=int, default=1000)
    ap.add_argument("--procs", type=int, default=32)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--timed", type=int, default=20)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "procset", "rate.json"))
    a = ap.parse_args()
    L = _lib.load()
    ctx = _lib.Context(0)
    S, E, P = a.seeds, a.events, a.procs
    evhash = splitmix64(0x5EED5, E)
    evclass = np.where(np.arange(E) % 16 < 4, _lib.NMZ_EV_PRIORITIZED, 0).astype(np.uint8)
    n_procs = np.full(E, P, np.uint32)
    target = np.full(E, P // 2, np.uint32)
    record = {"workload": {"seeds": S, "events": E, "procs_per_event": P, "interval_ns": [30_000_000, 100_000_000],
                           "warmup_sweeps": a.warmup, "timed_sweeps": a.timed, "repetitions": a.reps},
              "timing": "device events around k_procset_sweep; every sweep call ends in a stream synchronise",
              "k2_context": K2_CONTEXT, "policies": {}}
    tot, cnt = ctypes.c_double(), ctypes.c_uint64()
    for name in ("mild", "extreme", "dirichlet"):
        p = Random()
        p.MinInterval, p.MaxInterval, p.ProcPolicy = 30_000_000, 100_000_000, name
        # one sweep with statistics: the outputs the decisions consume (re-draws, <= 2.4e-7 per draw, not counted)
        r = p.ProcSetSweep(0, S, evhash, evclass, n_procs, target, k=8, ctx=ctx)
        draws = S * E * P if name != "extreme" else S * E * 3 + int(r.stats["n_special"].sum(dtype=np.uint64))
        outputs = S * E + draws
        ms = []
        for _ in range(a.reps):
            for _ in range(a.warmup):
                p.ProcSetSweep(0, S, evhash, evclass, n_procs, target, ctx=ctx)
            _lib.check(L.nmz_timing_enable(ctx.handle, 1))
            L.nmz_timing_read(ctx.handle, b"procset_sweep", ctypes.byref(tot), ctypes.byref(cnt), 1)
            for _ in range(a.timed):
                p.ProcSetSweep(0, S, evhash, evclass, n_procs, target, ctx=ctx)
            _lib.check(L.nmz_timing_read(ctx.handle, b"procset_sweep", ctypes.byref(tot), ctypes.byref(cnt), 1))
            _lib.check(L.nmz_timing_enable(ctx.handle, 0))
            assert cnt.value == a.timed
            ms.append(tot.value / cnt.value)
        med = float(np.median(ms))
        record["policies"][name] = {
            "kernel_ms_per_sweep": ms, "median_ms": med, "spread": (max(ms) - min(ms)) / med,
            "process_decisions_per_s": S * E * P / med * 1e3, "outputs_per_sweep": outputs,
            "outputs_per_s": outputs / med * 1e3, "top_target_score": int(r.topk["target_score"][0])}
        print(f"{name}: {med:.3f} ms/sweep  {S * E * P / med * 1e3:.4g} process-decisions/s  "
              f"{outputs / med * 1e3:.4g} outputs/s  spread {(max(ms) - min(ms)) / med:.3%}", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(record, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
