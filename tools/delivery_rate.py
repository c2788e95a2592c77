"""Delivery-sweep rate (a tool, not a bench leg): decimal seeds over the configs[1] hint table, maxInterval 100 ms.

Measured, profiler off:
  (a) sweep + classes (nmz_replayable_delivery_sweep_decimal_dev + nmz_delivery_classes_dev, back to back on one
      stream) at 2^16 and 2^20 seeds x E in {64, 1,024, 4,096}, exact mode and PO mode with 16 entities: one warm-up,
      then `--reps` windows, each ended by a synchronise and sized to about `--window` seconds (host clock).
      Reported: the median ms per sweep + classes, the spread over the windows, seeds/s and sorted keys/s.
  (b) the parent route at 2^16 seeds x 1,024 events, PO, 16 entities, host arrays to a host first_equal: the only
      route before the delivery sweep existed -- nmz_replayable_sweep with every seed's delays dumped (512 MB to the
      host), a numpy stable argsort of every row, the permuted traces, nmz_unique_traces -- against
      nmz_replayable_delivery_sweep_decimal, alternating, results compared; medians of `--reps`.
Then a second run of (a)'s smaller shapes under `rocprofv3 --kernel-trace --stats` (its own child process) leaves the
kernels' shares next to the record.
usage: python3 tools/delivery_rate.py [--out profiles/delivery/rate.json] [--no-profile]
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
from namazu_amd.explorepolicy import to_csr  # noqa: E402
from namazu_amd.synth import splitmix64  # noqa: E402

M = 100_000_000
N_ENT = 16


def trace(E, po):
    """bench.py's configs[1] hint table (decimal signed int64, ZooKeeper-style replay hints), arrivals 25 us apart,
    symbols from the same generator, entities round-robin."""
    hints = [str(int(x)) for x in splitmix64(0x5EED, E).view(np.int64)]
    sym = splitmix64(0xD311, E)
    ent = (np.arange(E) % N_ENT).astype(np.uint32) if po else None
    return hints, np.arange(E, dtype=np.int64) * 25_000, sym, ent


def p(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


def windows(step, sync, reps, window_s):
    step()
    sync()
    t0 = time.perf_counter()
    step()
    sync()
    n = int(min(2000, max(1, window_s / max(time.perf_counter() - t0, 1e-6))))
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
    for S in a.seeds:
        d_st = torch.zeros(S * 32, dtype=torch.uint8, device="cuda")
        d_fe = torch.zeros(S, dtype=torch.int32, device="cuda")
        d_rep = torch.zeros(S, dtype=torch.int32, device="cuda")
        d_nc = torch.zeros(1, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        for E in a.events:
            for po in (False, True):
                hints, arrival, sym, ent = trace(E, po)
                hoff, hb = to_csr(hints)
                plan = ctypes.c_void_p()
                _lib.check(L.nmz_replayable_delivery_plan_create(ctx.handle, p(hoff), p(hb), E, M, p(arrival), p(sym),
                                                                 p(ent), S, ctypes.byref(plan)))

                def step():
                    _lib.check(L.nmz_replayable_delivery_sweep_decimal_dev(plan, 0, S,
                                                                           ctypes.c_void_p(d_st.data_ptr()), st))
                    _lib.check(L.nmz_delivery_classes_dev(ctx.handle, ctypes.c_void_p(d_st.data_ptr()), S,
                                                          ctypes.c_void_p(d_fe.data_ptr()),
                                                          ctypes.c_void_p(d_rep.data_ptr()),
                                                          ctypes.c_void_p(d_nc.data_ptr()), st))
                if profile:
                    for _ in range(2):
                        step()
                    stream.synchronize()
                else:
                    r = windows(step, stream.synchronize, a.reps, a.window)
                    r.update(seeds=S, events=E, mode="po16" if po else "exact", n_classes=int(d_nc.cpu()[0]),
                             seeds_per_s=S / r["median_ms"] * 1e3, keys_per_s=S * E / r["median_ms"] * 1e3)
                    out[f"seeds_{S}_E{E}_{r['mode']}"] = r
                    print(f"S={S} E={E} {r['mode']}: {r['median_ms']:.3f} ms  {r['seeds_per_s']:.4g} seeds/s  "
                          f"{r['keys_per_s']:.4g} keys/s  classes {r['n_classes']}  spread {r['spread']:.2%}",
                          flush=True)
                _lib.check(L.nmz_replayable_delivery_plan_destroy(plan))
    return out


def parent_route(a, L, ctx):
    """2^16 seeds x 1,024 events, PO with 16 entities, to a host first_equal."""
    S, E = a.gate_seeds, a.gate_events
    hints, arrival, sym, ent = trace(E, True)
    hoff, hb = to_csr(hints)
    soff, sb = to_csr([str(i) for i in range(S)])
    delays = np.zeros((S, E), np.int64)
    off = np.arange(S + 1, dtype=np.uint64) * np.uint64(E)
    parts = {}

    def old():
        t0 = time.perf_counter()
        _lib.check(L.nmz_replayable_sweep(ctx.handle, p(soff), p(sb), S, p(hoff), p(hb), E, M, None, p(delays), S, 0,
                                          None))
        t1 = time.perf_counter()
        order = np.argsort(delays + arrival[None, :], axis=1, kind="stable")  # ties by event index
        t2 = time.perf_counter()
        sy, en = np.ascontiguousarray(sym[order].reshape(-1)), np.ascontiguousarray(ent[order].reshape(-1))
        fe = np.zeros(S, np.uint32)
        _lib.check(L.nmz_unique_traces(ctx.handle, p(off), p(sy), p(en), S, p(fe)))
        t3 = time.perf_counter()
        parts.setdefault("dump_ms", []).append((t1 - t0) * 1e3)
        parts.setdefault("argsort_ms", []).append((t2 - t1) * 1e3)
        parts.setdefault("permute_and_unique_ms", []).append((t3 - t2) * 1e3)
        return fe

    def new():
        fe = np.zeros(S, np.uint32)
        _lib.check(L.nmz_replayable_delivery_sweep_decimal(ctx.handle, 0, S, p(hoff), p(hb), E, M, p(arrival), p(sym),
                                                           p(ent), None, p(fe), None, None))
        return fe

    for f in (old, new):  # warm-up: page faults of the 512 MB, code objects
        f()
    parts.clear()
    t_old, t_new = [], []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        ro = old()
        t1 = time.perf_counter()
        rn = new()
        t2 = time.perf_counter()
        t_old.append((t1 - t0) * 1e3)
        t_new.append((t2 - t1) * 1e3)
        assert np.array_equal(ro, rn), "the two routes disagree"
    mo, mn = float(np.median(t_old)), float(np.median(t_new))
    r = {"seeds": S, "events": E, "entities": N_ENT, "delay_bytes_to_host": S * E * 8, "parent_route_ms": t_old,
         "parent_route_parts_ms": parts, "delivery_sweep_ms": t_new, "parent_route_median_ms": mo,
         "delivery_sweep_median_ms": mn, "ratio": mo / mn, "bar": 10.0, "bar_met": mo / mn >= 10.0,
         "n_classes": int((rn == np.arange(S)).sum()), "results_equal": True,
         "what": "end to end from host arrays to a host first_equal, each call creating its own plan; parent route = "
                 "nmz_replayable_sweep(n_dump_seeds = n_seeds) + numpy stable argsort + permuted traces + "
                 "nmz_unique_traces, new = nmz_replayable_delivery_sweep_decimal(first_equal only)"}
    print(f"parent route {mo:.1f} ms, delivery sweep {mn:.2f} ms, ratio {mo / mn:.1f}x", flush=True)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", type=int, nargs="+", default=[1 << 16, 1 << 20])
    ap.add_argument("--events", type=int, nargs="+", default=[64, 1024, 4096])
    ap.add_argument("--gate-seeds", type=int, default=1 << 16)
    ap.add_argument("--gate-events", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.25)
    ap.add_argument("--mode", choices=["main", "profile"], default="main")
    ap.add_argument("--no-profile", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "delivery", "rate.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("delivery_rate.py measures on the GPU; no device found")
    L = _lib.load()
    ctx = _lib.Context(0)
    if a.mode == "profile":
        rate_configs(a, L, ctx, torch, True)
        return
    record = {"workload": {"hints": "configs[1] table (bench.py zk_hints)", "max_interval_ns": M,
                           "arrival_spacing_ns": 25_000, "po_entities": N_ENT, "windows": a.reps,
                           "window_seconds": a.window},
              "timing": "host clock around back-to-back sweep + classes on one stream, each window ended by a "
                        "synchronise; profiler off",
              "sweep_and_classes": rate_configs(a, L, ctx, torch, False),
              "parent_route": parent_route(a, L, ctx)}
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(record, f, indent=1, sort_keys=True)
        f.write("\n")
    if a.no_profile:
        return
    tmp = tempfile.mkdtemp(prefix="delivery_prof_")
    try:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "-o", "run", "--"] + \
            [sys.executable, os.path.abspath(__file__), "--mode", "profile", "--seeds", str(a.seeds[0]), "--events"] + \
            [str(e) for e in a.events]
        prof = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        found = glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True)
        if prof.returncode != 0 or not found:
            sys.exit("profile run failed:\n" + prof.stderr[-2000:])
        shutil.copy(found[0], os.path.join(os.path.dirname(os.path.abspath(a.out)), "kernel_stats.csv"))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
