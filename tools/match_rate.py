"""Run-matching rate (a tool, not a bench leg): nmz_match_runs_dev over generated storages of E events x R runs with
run length E (tests/match_cases.py's shape: E // 4 distinct symbols with repeats and arrival ties; every run misses
20 % of the events and carries E // 10 unknown symbols and E // 10 duplicates), beside nmz_order_contrast_dev
(d_counts == NULL, k = 64) over the rows the match just made, in the same run.

Measured, profiler off:
  * E in {1,024, 4,096} x R in {256, 4,096}: a few warm-up calls, then `--reps` windows of back-to-back calls on one
    stream, each window ended by a synchronise and sized to about `--window` seconds (host clock), first for the
    match, then for the contrast. Reported: the median ms per call and the spread of each, run elements/s of the
    match, and match time over contrast time. The acceptance relation -- at E = 4,096 the match takes no longer than
    the contrast it feeds -- is recorded per shape (`match_within_contrast`), not tuned. Before the timing the first
    rows of the device result are compared with historystorage.run_positions.
  * the parent's only route, historystorage.run_positions (numpy on the host), against nmz_match_runs at E = 1,024,
    R = 256, host arrays to a host pos, alternating, equal results asserted, medians of `--reps`. Recorded, not gated.
usage: python3 tools/match_rate.py [--out profiles/match/rate.json]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import match_cases as M  # noqa: E402
from namazu_amd import _lib, historystorage as hs  # noqa: E402
from order_rate import windows  # noqa: E402

K = 64
CHECK_ROWS = 8


def storage(E, R, seed):
    """(sym, arrival, runs): a match_cases universe of E events over E // 4 symbols and R runs of length E."""
    rng = np.random.default_rng(seed)
    sym, arrival = M.universe(E, max(1, E // 4), rng)
    return sym, arrival, [M.run(sym, E, rng) for _ in range(R)]


def rate_configs(a, L, ctx, torch):
    out = {}
    stream = torch.cuda.Stream()
    st = ctypes.c_void_p(stream.cuda_stream)
    d_pairs = torch.zeros(K * 32, dtype=torch.uint8, device="cuda")
    d_info = torch.zeros(16, dtype=torch.uint8, device="cuda")
    for E in a.events:
        for R in a.runs:
            sym, arrival, runs = storage(E, R, 1000 * E + R)
            ts = hs.TraceSet(runs)
            plan = hs.MatchPlan(sym, arrival, ctx=ctx)
            d_off = torch.from_numpy(ts.off.view(np.int64)).cuda()
            d_sym = torch.from_numpy(ts.sym.view(np.int64)).cuda()
            d_pos = torch.zeros((R, E), dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()

            def match():
                plan.runs_dev(d_off.data_ptr(), d_sym.data_ptr(), R, d_pos.data_ptr(), stream.cuda_stream)

            match()
            stream.synchronize()
            head = d_pos[:CHECK_ROWS].cpu().numpy().view(np.uint32)
            assert np.array_equal(head, hs.run_positions(sym, arrival, runs[:CHECK_ROWS])), "the match is wrong"
            # labels planted on one pair with 10 % noise, as tests/contrast_ref.gen plants them
            p64 = d_pos.to(torch.int64) & 0xFFFFFFFF
            g = torch.Generator(device="cuda")
            g.manual_seed(E + R)
            noise = torch.rand(R, generator=g, device="cuda") < 0.10
            failed = ((p64[:, 7 % E] < p64[:, 3 % E]) ^ noise).to(torch.uint8)
            failed[0], failed[-1] = 1, 0
            failed = failed.contiguous()
            del p64
            torch.cuda.synchronize()

            def contrast():
                _lib.check(L.nmz_order_contrast_dev(ctx.handle, ctypes.c_void_p(d_pos.data_ptr()),
                                                    ctypes.c_void_p(failed.data_ptr()), R, E, K, None,
                                                    ctypes.c_void_p(d_pairs.data_ptr()),
                                                    ctypes.c_void_p(d_info.data_ptr()), st))

            m = windows(match, stream.synchronize, a.warmup, a.reps, a.window)
            c = windows(contrast, stream.synchronize, a.warmup, a.reps, a.window)
            elems = int(ts.off[-1])
            r = {"events": E, "runs": R, "symbols": plan.n_symbols, "run_elements": elems, "match": m, "contrast": c,
                 "run_elements_per_s": elems / m["median_ms"] * 1e3,
                 "match_over_contrast": m["median_ms"] / c["median_ms"],
                 "match_within_contrast": bool(m["median_ms"] <= c["median_ms"]),
                 "matched_cells": float((head != M.NONE).mean()), "rows_checked": CHECK_ROWS}
            out[f"E{E}_R{R}"] = r
            print(f"E={E} R={R}: match {m['median_ms']:.4f} ms/call (spread {m['spread']:.2%}, "
                  f"{r['run_elements_per_s']:.4g} elements/s)  contrast {c['median_ms']:.4f} ms/call "
                  f"(spread {c['spread']:.2%})  match / contrast {r['match_over_contrast']:.3f}"
                  + ("" if r["match_within_contrast"] or E != 4096 else "  ACCEPTANCE MISSED"), flush=True)
            plan.close()
            del d_off, d_sym, d_pos, failed
    return out


def host_route(a, ctx):
    """E = 1,024, R = 256, host arrays to a host pos: run_positions (numpy) against nmz_match_runs."""
    E, R = a.gate_events, a.gate_runs
    sym, arrival, runs = storage(E, R, 1000 * E + R)

    def old():
        return hs.run_positions(sym, arrival, runs)

    def new():
        return hs.match_runs(sym, arrival, runs, ctx=ctx)

    for f in (old, new):
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
        assert ro.tobytes() == rn.tobytes(), "the two routes disagree"
    mo, mn = float(np.median(t_old)), float(np.median(t_new))
    print(f"run_positions {mo:.1f} ms, nmz_match_runs {mn:.3f} ms, ratio {mo / mn:.1f}x", flush=True)
    return {"events": E, "runs": R, "run_positions_ms": t_old, "match_runs_ms": t_new, "run_positions_median_ms": mo,
            "match_runs_median_ms": mn, "ratio": mo / mn, "results_equal": True,
            "what": "end to end from host arrays (a list of runs) to a host pos[R][E]; run_positions = numpy "
                    "match_target per run, match_runs = CSR packing + nmz_match_runs (plan, upload, kernel, download)"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--events", type=int, nargs="+", default=[1024, 4096])
    ap.add_argument("--runs", type=int, nargs="+", default=[256, 4096])
    ap.add_argument("--gate-events", type=int, default=1024)
    ap.add_argument("--gate-runs", type=int, default=256)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.25)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "match", "rate.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("match_rate.py measures on the GPU; no device found")
    L = _lib.load()
    ctx = _lib.Context(0)
    record = {"workload": {"storage": "tests/match_cases.py's shape: E // 4 symbols, runs of length E", "k": K,
                           "d_counts": None, "warmup_calls": a.warmup, "windows": a.reps,
                           "window_seconds": a.window},
              "timing": "host clock around back-to-back calls on one stream, each window ended by a synchronise; "
                        "profiler off",
              "match_and_contrast": rate_configs(a, L, ctx, torch),
              "host_route": host_route(a, ctx)}
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(record, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
