"""Order-contrast rate (a tool, not a bench leg): nmz_order_contrast_dev with d_counts == NULL (the hot form), k = 64,
over generated storages of E events x R runs (tests/contrast_ref.py's shape: a random order per run, 15 % of the
cells absent, labels planted on one pair with 10 % noise; generated on the device).

Measured, profiler off:
  * E in {1,024, 4,096} x R in {256, 4,096, 65,535}: a few warm-up calls, then `--reps` windows of back-to-back calls
    on one stream, each window ended by a synchronise and sized to about `--window` seconds (host clock). Reported:
    the median ms per call, the spread over the windows, predicates/s (E^2 R per call), and beside each time the
    time this design takes at issue peak,
        E^2 R x (issue cycles per wave-wide compare-and-count) / (1,024 SIMDs x 64 lanes x 2.4 GHz),
    with 6.3 cycles = v_cmp with an SGPR operand (half rate, 4.1) + VCC-carry v_addc_co (full rate, 2.2), the forms
    the sweep's ISA shows, at tools/ubench's costs ("Issue costs"). The gap is recorded, not
    gated.
  * the only earlier route, the numpy restatement on the host (tests/contrast_ref.py), against nmz_order_contrast at
    E = 1,024, R = 256, host arrays to a host top-64, alternating, equal results, medians of `--reps`. Gate: the
    ratio must exceed 1.
Then a second run of the same calls under `rocprofv3 --kernel-trace --stats` (its own child process: tracing slows
the host) leaves the kernels' statistics next to the record.
usage: python3 tools/contrast_rate.py [--out profiles/contrast/rate.json] [--no-profile]
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
import contrast_ref as C  # noqa: E402
from namazu_amd import _lib, historystorage as hs  # noqa: E402
from order_rate import windows  # noqa: E402

K = 64
ISSUE_CYCLES = 6.3                  # v_cmp with an SGPR operand 4.1 + v_addc_co 2.2 (tools/ubench)
LANES_PER_S = 1024 * 64 * 2.4e9     # SIMDs x lanes x clock


def storage(torch, E, R, seed):
    """pos[R][E] uint32 and failed[R] uint8 on the device, in the shape of tests/contrast_ref.gen."""
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    pos = torch.empty((R, E), dtype=torch.int64, device="cuda")
    step = max(1, (1 << 26) // E)  # rows per piece: the sort's temporaries stay small
    for r0 in range(0, R, step):
        n = min(step, R - r0)
        pos[r0:r0 + n] = torch.argsort(torch.rand((n, E), generator=g, device="cuda"), dim=1) * 3 + 1
    absent = torch.rand((R, E), generator=g, device="cuda") < 0.15
    absent[:, 7 % E] = False
    absent[:, 3 % E] = False
    noise = torch.rand(R, generator=g, device="cuda") < 0.10
    failed = ((pos[:, 7 % E] < pos[:, 3 % E]) ^ noise).to(torch.uint8)
    failed[0], failed[-1] = 1, 0
    pos[absent] = C.NONE
    # uint32 bit patterns in an int32 tensor: the library reads the bytes
    pos32 = (pos & 0xFFFFFFFF).to(torch.int64)
    pos32 = torch.where(pos32 >= (1 << 31), pos32 - (1 << 32), pos32).to(torch.int32).contiguous()
    return pos32, failed.contiguous()


def rate_configs(a, L, ctx, torch, profile):
    out = {}
    stream = torch.cuda.Stream()
    st = ctypes.c_void_p(stream.cuda_stream)
    d_pairs = torch.zeros(K * 32, dtype=torch.uint8, device="cuda")
    d_info = torch.zeros(16, dtype=torch.uint8, device="cuda")
    for E in a.events:
        for R in a.runs:
            pos, failed = storage(torch, E, R, 1000 * E + R)
            torch.cuda.synchronize()

            def step():
                _lib.check(L.nmz_order_contrast_dev(ctx.handle, ctypes.c_void_p(pos.data_ptr()),
                                                    ctypes.c_void_p(failed.data_ptr()), R, E, K, None,
                                                    ctypes.c_void_p(d_pairs.data_ptr()),
                                                    ctypes.c_void_p(d_info.data_ptr()), st))
            if profile:
                for _ in range(3):
                    step()
                stream.synchronize()
            else:
                r = windows(step, stream.synchronize, a.warmup, a.reps, a.window)
                pred = float(E) * E * R
                peak_ms = pred * ISSUE_CYCLES / LANES_PER_S * 1e3
                info = np.frombuffer(d_info.cpu().numpy().tobytes(), _lib.CONTRAST_INFO_DTYPE)[0]
                best = np.frombuffer(d_pairs.cpu().numpy().tobytes(), _lib.ORDER_PAIR_DTYPE)[0]
                r.update(events=E, runs=R, predicates=pred, predicates_per_s=pred / r["median_ms"] * 1e3,
                         issue_peak_ms=peak_ms, time_over_issue_peak=r["median_ms"] / peak_ms,
                         n_positive=int(info["n_positive"]), best_pair=[int(best["before"]), int(best["after"])])
                out[f"E{E}_R{R}"] = r
                print(f"E={E} R={R}: {r['median_ms']:.4f} ms/call  {r['predicates_per_s']:.4g} predicates/s  "
                      f"issue peak {peak_ms:.4f} ms ({r['time_over_issue_peak']:.2f}x)  spread {r['spread']:.2%}",
                      flush=True)
            del pos, failed
    return out


def numpy_route(a, ctx):
    """E = 1,024, R = 256, host arrays to a host top-64: the numpy restatement against nmz_order_contrast."""
    E, R = a.gate_events, a.gate_runs
    pos, failed = C.gen(E, R, 1000 * E + R)

    def old():
        F, P = C.counts(pos, failed)
        return C.ranked(F, P, failed, K)

    def new():
        r = hs.order_contrast(pos, failed, k=K, ctx=ctx)
        return r.pairs, r.n_positive

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
        assert ro[1] == rn[1] and ro[0].tobytes() == rn[0].tobytes(), "the two routes disagree"
    mo, mn = float(np.median(t_old)), float(np.median(t_new))
    print(f"numpy restatement {mo:.1f} ms, order contrast {mn:.3f} ms, ratio {mo / mn:.1f}x", flush=True)
    if not mo / mn > 1:
        sys.exit("gate: the device route is not faster than the numpy restatement")
    return {"events": E, "runs": R, "k": K, "numpy_ms": t_old, "order_contrast_ms": t_new, "numpy_median_ms": mo,
            "order_contrast_median_ms": mn, "ratio": mo / mn, "results_equal": True,
            "what": "end to end from host arrays to a host top-64; numpy = tests/contrast_ref.py counts + ranked, "
                    "order contrast = nmz_order_contrast(counts = NULL)"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--events", type=int, nargs="+", default=[1024, 4096])
    ap.add_argument("--runs", type=int, nargs="+", default=[256, 4096, 65535])
    ap.add_argument("--gate-events", type=int, default=1024)
    ap.add_argument("--gate-runs", type=int, default=256)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.25)
    ap.add_argument("--mode", choices=["main", "profile"], default="main")
    ap.add_argument("--no-profile", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "contrast", "rate.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("contrast_rate.py measures on the GPU; no device found")
    L = _lib.load()
    ctx = _lib.Context(0)
    if a.mode == "profile":
        rate_configs(a, L, ctx, torch, True)
        return
    record = {"workload": {"storage": "tests/contrast_ref.gen's shape, generated on the device", "k": K,
                           "d_counts": None, "warmup_calls": a.warmup, "windows": a.reps,
                           "window_seconds": a.window},
              "timing": "host clock around back-to-back calls on one stream, each window ended by a synchronise; "
                        "profiler off",
              "issue_peak": {"cycles_per_wave_compare_and_count": ISSUE_CYCLES,
                             "forms": "v_cmp_lt_u32 with an SGPR operand 4.1 + v_addc_co_u32 2.2 (tools/ubench)",
                             "lanes_per_s": LANES_PER_S},
              "order_contrast": rate_configs(a, L, ctx, torch, False),
              "numpy_route": numpy_route(a, ctx)}
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    if os.path.exists(a.out):  # keep what other tools recorded next to the rates (the headline runs)
        with open(a.out) as f:
            old = json.load(f)
        for k in old:
            record.setdefault(k, old[k])
    with open(a.out, "w") as f:
        json.dump(record, f, indent=1, sort_keys=True)
        f.write("\n")
    if a.no_profile:
        return
    tmp = tempfile.mkdtemp(prefix="contrast_prof_")
    try:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "-o", "run", "--"] + \
            [sys.executable, os.path.abspath(__file__), "--mode", "profile", "--events"] + \
            [str(e) for e in a.events] + ["--runs"] + [str(r) for r in a.runs]
        prof = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        found = glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True)
        if prof.returncode != 0 or not found:
            sys.exit("profile run failed:\n" + prof.stderr[-2000:])
        shutil.copy(found[0], os.path.join(os.path.dirname(os.path.abspath(a.out)), "kernel_stats.csv"))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
