"""Order-sweep rate (a tool, not a bench leg): decimal seeds over the configs[1] hint table against C event-order
constraints, top-64 only (d_stats == NULL, the hot form).

Measured, profiler off:
  * 2^20 and 2^24 seeds x C in {8, 64}, maxInterval 100 ms, k = 64: a few warm-up sweeps, then `--reps` windows of
    back-to-back sweeps on one stream, each window ended by a synchronise and sized to about `--window` seconds (host
    clock). Reported: the median ms per sweep, the spread over the windows, seeds/s and delay evaluations/s (2 C per
    seed).
  * for context (not a gate), the existing per-decision sweep over the same trace in decisions/s, from a child process
    whose plan is created under NMZ_AB=1 NMZ_REPLAY_WT=0 NMZ_REPLAY_OQ=0 (no wavelet trees, no order queries).
  * the parent-route comparison at 2^16 seeds x 1,024 events, C = 8, end to end to a host top-64: the only route
    before the order sweep existed -- nmz_replayable_sweep with every seed's delays dumped (512 MB to the host) and
    the constraints filtered in numpy -- against nmz_replayable_order_sweep_decimal with stats == NULL, alternating,
    both results compared.
Then a second run of the same sweeps under `rocprofv3 --kernel-trace --stats` (its own child process: tracing slows
the host) leaves the kernels' statistics next to the record.
usage: python3 tools/order_rate.py [--out profiles/order/rate.json] [--no-profile]
"""
import argparse
import ctypes
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
from namazu_amd import _lib  # noqa: E402
from namazu_amd.explorepolicy import Replayable, to_csr  # noqa: E402
from namazu_amd.synth import splitmix64  # noqa: E402

M = 100_000_000
K = 64


def zk_hints(n_events, seed=0x5EED):
    """bench.py's configs[1] hint table: decimal signed int64 (ZooKeeper-style replay hints)."""
    return [str(int(x)) for x in splitmix64(seed, n_events).view(np.int64)]


def trace(E, C):
    """Hints, arrivals 25 us apart and C constraints over random distinct pairs with a 1 ms margin."""
    rng = np.random.default_rng(E * 131 + C)
    cons = []
    while len(cons) < C:
        b, a = (int(x) for x in rng.integers(0, E, 2))
        if b != a:
            cons.append((b, a, 1_000_000))
    return zk_hints(E), np.arange(E, dtype=np.int64) * 25_000, Replayable.order_constraints(cons)


def p(a):
    return ctypes.c_void_p(a.ctypes.data)


class OrderPlan:
    def __init__(self, L, ctx, E, C, max_seeds):
        hints, arrival, cons = trace(E, C)
        hoff, hb = to_csr(hints)
        self.L, self.h = L, ctypes.c_void_p()
        _lib.check(L.nmz_replayable_order_plan_create(ctx.handle, p(hoff), p(hb), E, M, p(arrival), p(cons), C,
                                                      max_seeds, ctypes.byref(self.h)))

    def close(self):
        _lib.check(self.L.nmz_replayable_order_plan_destroy(self.h))


def windows(step, sync, warmup, reps, window_s):
    """ms per step: `reps` windows of back-to-back steps, each ended by a synchronise."""
    for _ in range(warmup):
        step()
    sync()
    t0 = time.perf_counter()
    step()
    sync()
    n = int(min(2000, max(3, window_s / max(time.perf_counter() - t0, 1e-6))))
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        for _ in range(n):
            step()
        sync()
        ms.append((time.perf_counter() - t0) / n * 1e3)
    med = float(np.median(ms))
    return {"ms_per_sweep": ms, "median_ms": med, "spread": (max(ms) - min(ms)) / med, "sweeps_per_window": n}


def rate_configs(a, L, ctx, torch, profile):
    out = {}
    stream = torch.cuda.Stream()
    st = ctypes.c_void_p(stream.cuda_stream)
    d_tk = torch.zeros(K * 24, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    for S in a.seeds:
        for C in (8, 64):
            plan = OrderPlan(L, ctx, a.events, C, S)

            def step():
                _lib.check(L.nmz_replayable_order_sweep_decimal_dev(plan.h, 0, S, K, None,
                                                                    ctypes.c_void_p(d_tk.data_ptr()), st))
            if profile:
                for _ in range(3):
                    step()
                stream.synchronize()
            else:
                r = windows(step, stream.synchronize, a.warmup, a.reps, a.window)
                r.update(seeds=S, constraints=C, seeds_per_s=S / r["median_ms"] * 1e3,
                         delay_evaluations_per_s=2 * C * S / r["median_ms"] * 1e3)
                out[f"seeds_{S}_C{C}"] = r
                print(f"S={S} C={C}: {r['median_ms']:.4f} ms/sweep  {r['seeds_per_s']:.4g} seeds/s  "
                      f"{r['delay_evaluations_per_s']:.4g} delay evaluations/s  spread {r['spread']:.2%}", flush=True)
            plan.close()
    return out


def per_decision(a, L, ctx, torch):
    """Child process (NMZ_AB=1 NMZ_REPLAY_WT=0 NMZ_REPLAY_OQ=0): the per-decision sweep of the same trace."""
    S, E = a.seeds[0], a.events
    hoff, hb = to_csr(zk_hints(E))
    plan = ctypes.c_void_p()
    _lib.check(L.nmz_replayable_plan_create(ctx.handle, p(hoff), p(hb), E, M, S, ctypes.byref(plan)))
    kind = L.nmz_replayable_plan_kernel(plan)
    stream = torch.cuda.Stream()
    st = ctypes.c_void_p(stream.cuda_stream)
    d_st = torch.zeros(S * 32, dtype=torch.uint8, device="cuda")
    d_tk = torch.zeros(K * 24, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()

    def step():
        _lib.check(L.nmz_replayable_sweep_decimal_topk_dev(plan, 0, S, K, ctypes.c_void_p(d_st.data_ptr()),
                                                           ctypes.c_void_p(d_tk.data_ptr()), st))
    r = windows(step, stream.synchronize, a.warmup, a.reps, a.window)
    L.nmz_replayable_plan_destroy(plan)
    # as bench.py's k1_kernel: the plan still builds its order-query images (kind 1), but with NMZ_REPLAY_OQ=0 and
    # maxInterval < 2^30 its sweeps take the per-decision kernel
    per_decision = os.environ.get("NMZ_AB") == "1" and os.environ.get("NMZ_REPLAY_OQ") == "0" and M < (1 << 30)
    kernel = "k_replayable_sweep_fast" if per_decision else \
        {2: "k_replayable_sweep_wt", 1: "k_replayable_sweep_oq", 0: "k_replayable_sweep_fast"}[kind]
    r.update(seeds=S, events=E, plan_kernel=kind, kernel=kernel, decisions_per_s=S * E / r["median_ms"] * 1e3)
    print(json.dumps(r))


def parent_route(a, L, ctx):
    """2^16 seeds x 1,024 events, C = 8, to a host top-64: dump + numpy filter against the order sweep."""
    S, E, C = a.gate_seeds, a.gate_events, 8
    hints, arrival, cons = trace(E, C)
    hoff, hb = to_csr(hints)
    soff, sb = to_csr([str(i) for i in range(S)])
    delays = np.zeros((S, E), np.int64)
    topk = np.zeros(K, _lib.TOPK_DTYPE)

    def old():
        _lib.check(L.nmz_replayable_sweep(ctx.handle, p(soff), p(sb), S, p(hoff), p(hb), E, M, None, p(delays), S, 0,
                                          None))
        # only the 2 C columns the constraints name are read (no pass over the whole dump)
        sl = (delays[:, cons["after"]] + arrival[cons["after"]]) - (delays[:, cons["before"]] + arrival[cons["before"]]) \
            - cons["margin_ns"][None, :]
        n_sat, mn = (sl >= 0).sum(axis=1), sl.min(axis=1)
        order = np.lexsort((np.arange(S), -mn, -n_sat))[:K]
        return order, n_sat[order], mn[order], sl[order].argmin(axis=1)

    def new():
        _lib.check(L.nmz_replayable_order_sweep_decimal(ctx.handle, 0, S, p(hoff), p(hb), E, M, p(arrival), p(cons), C,
                                                        K, None, p(topk)))
        return topk["seed"].astype(np.int64), topk["n_fault"], topk["sum_delay_ns"], topk["first_fault"]

    for f in (old, new):  # warm-up: page faults of the 512 MB, code objects
        f()
    t_old, t_new = [], []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        ro = old()
        t1 = time.perf_counter()
        rn = new()
        t2 = time.perf_counter()
        t_old.append((t1 - t0) * 1e3)
        t_new.append((t2 - t1) * 1e3)
        assert all(np.array_equal(x, y) for x, y in zip(ro, rn)), "the two routes disagree"
    mo, mn_ = float(np.median(t_old)), float(np.median(t_new))
    r = {"seeds": S, "events": E, "constraints": C, "k": K, "delay_bytes_to_host": S * E * 8,
         "parent_route_ms": t_old, "order_sweep_ms": t_new, "parent_route_median_ms": mo,
         "order_sweep_median_ms": mn_, "ratio": mo / mn_, "results_equal": True,
         "what": "end to end from host arrays to a host top-64, each call creating its own plan; parent route = "
                 "nmz_replayable_sweep(n_dump_seeds = n_seeds) + numpy filter, order sweep = "
                 "nmz_replayable_order_sweep_decimal(stats = NULL)"}
    print(f"parent route {mo:.2f} ms, order sweep {mn_:.3f} ms, ratio {mo / mn_:.1f}x", flush=True)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", type=int, nargs="+", default=[1 << 20, 1 << 24])
    ap.add_argument("--events", type=int, default=4096)
    ap.add_argument("--gate-seeds", type=int, default=1 << 16)
    ap.add_argument("--gate-events", type=int, default=1024)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.25)
    ap.add_argument("--mode", choices=["main", "profile", "per-decision"], default="main")
    ap.add_argument("--no-profile", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "order", "rate.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("order_rate.py measures on the GPU; no device found")
    L = _lib.load()
    ctx = _lib.Context(0)
    if a.mode == "per-decision":
        return per_decision(a, L, ctx, torch)
    if a.mode == "profile":
        rate_configs(a, L, ctx, torch, True)
        return
    record = {"workload": {"hints": "configs[1] table (bench.py zk_hints)", "events": a.events, "max_interval_ns": M,
                           "k": K, "d_stats": None, "warmup_sweeps": a.warmup, "windows": a.reps,
                           "window_seconds": a.window},
              "timing": "host clock around back-to-back sweeps on one stream, each window ended by a synchronise; "
                        "profiler off",
              "order_sweep": rate_configs(a, L, ctx, torch, False)}
    me = [sys.executable, os.path.abspath(__file__), "--seeds", str(a.seeds[0]), "--events", str(a.events),
          "--warmup", str(a.warmup), "--reps", str(a.reps), "--window", str(a.window)]
    env = dict(os.environ, NMZ_AB="1", NMZ_REPLAY_WT="0", NMZ_REPLAY_OQ="0")
    child = subprocess.run(me + ["--mode", "per-decision"], env=env, capture_output=True, text=True, timeout=600)
    if child.returncode != 0:
        sys.exit("per-decision child failed:\n" + child.stderr[-2000:])
    record["per_decision_sweep_context"] = json.loads(child.stdout.strip().splitlines()[-1])
    print(f"per-decision sweep: {record['per_decision_sweep_context']['decisions_per_s']:.4g} decisions/s", flush=True)
    record["parent_route"] = parent_route(a, L, ctx)
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(record, f, indent=1, sort_keys=True)
        f.write("\n")
    if a.no_profile:
        return
    tmp = tempfile.mkdtemp(prefix="order_prof_")
    try:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "-o", "run", "--"] + \
            [sys.executable, os.path.abspath(__file__), "--mode", "profile", "--events", str(a.events), "--seeds"] + \
            [str(s) for s in a.seeds]
        prof = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        found = glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True)
        if prof.returncode != 0 or not found:
            sys.exit("profile run failed:\n" + prof.stderr[-2000:])
        shutil.copy(found[0], os.path.join(os.path.dirname(os.path.abspath(a.out)), "kernel_stats.csv"))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
