"""Nearest-order sweep rate (a tool, not a bench leg): decimal seeds over the configs[1] hint table, maxInterval
100 ms, the target being the delivery order of a seed outside the swept range.

Measured, profiler off:
  (a) sweep + top-64 (nmz_replayable_target_sweep_decimal_dev, d_stats NULL) at 2^16 and 2^20 seeds x E in {64, 1,024,
      4,096}, exact mode and PO mode with 16 entities, and beside it the delivery sweep alone
      (nmz_replayable_delivery_sweep_decimal_dev) at the same shape in the same run: one warm-up, then `--reps`
      windows, each ended by a synchronise and sized to about `--window` seconds (host clock). Reported: the median
      ms of each, their ratio, seeds/s and sorted keys/s.
  (b) the only route before this sweep at 2^16 seeds x 1,024 events, exact mode, to the same top-64:
      nmz_replayable_sweep with every seed's delays dumped (512 MB to the host), a numpy stable argsort of every row
      and a numpy inversion count (one stable partition per bit of the rank) -- against
      nmz_replayable_target_sweep_decimal, results compared.
usage: python3 tools/target_rate.py [--out profiles/target/rate.json]
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from delivery_rate import M, N_ENT, p, trace, windows  # noqa: E402
from namazu_amd import _lib  # noqa: E402
from namazu_amd.explorepolicy import to_csr  # noqa: E402

K = 64
RECORDED = b"recorded-run"  # the seed whose order plays the recorded run; not a decimal string, so never swept


def recorded_target(L, hoff, hb, E, arrival, sym, ent):
    """target_pos of the order that seed RECORDED delivers (nmz_replayable_delivery_host)."""
    sb = np.frombuffer(RECORDED, np.uint8)
    order = np.zeros(E, np.uint32)
    _lib.check(L.nmz_replayable_delivery_host(p(sb), len(RECORDED), p(hoff), p(hb), E, M, p(arrival), p(sym), p(ent),
                                              None, p(order), None))
    tp = np.zeros(E, np.uint32)
    tp[order] = np.arange(E, dtype=np.uint32)
    return tp


def rate_configs(a, L, ctx, torch):
    out = {}
    stream = torch.cuda.Stream()
    st = ctypes.c_void_p(stream.cuda_stream)
    for S in a.seeds:
        d_st = torch.zeros(S * 32, dtype=torch.uint8, device="cuda")
        d_tk = torch.zeros(K * 24, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        for E in a.events:
            for po in (False, True):
                hints, arrival, sym, ent = trace(E, po)
                hoff, hb = to_csr(hints)
                tp = recorded_target(L, hoff, hb, E, arrival, sym, ent)
                tplan, dplan = ctypes.c_void_p(), ctypes.c_void_p()
                _lib.check(L.nmz_replayable_target_plan_create(ctx.handle, p(hoff), p(hb), E, M, p(arrival), p(ent),
                                                               p(tp), S, ctypes.byref(tplan)))
                _lib.check(L.nmz_replayable_delivery_plan_create(ctx.handle, p(hoff), p(hb), E, M, p(arrival), p(sym),
                                                                 p(ent), S, ctypes.byref(dplan)))

                def target():
                    _lib.check(L.nmz_replayable_target_sweep_decimal_dev(tplan, 0, S, 0, K, None,
                                                                         ctypes.c_void_p(d_tk.data_ptr()), st))

                def delivery():
                    _lib.check(L.nmz_replayable_delivery_sweep_decimal_dev(dplan, 0, S,
                                                                           ctypes.c_void_p(d_st.data_ptr()), st))
                r = windows(target, stream.synchronize, a.reps, a.window)
                d = windows(delivery, stream.synchronize, a.reps, a.window)
                best = np.frombuffer(d_tk.cpu().numpy().tobytes(), _lib.TOPK_DTYPE)[0]
                info = np.zeros(2, np.uint32)
                _lib.check(L.nmz_replayable_target_plan_info(tplan, p(info[0:1]), p(info[1:2])))
                r.update(seeds=S, events=E, mode="po16" if po else "exact", n_pairs=int(info[1]),
                         best_seed=int(best["seed"]), best_n_discordant=int(info[1]) - int(best["n_fault"]),
                         seeds_per_s=S / r["median_ms"] * 1e3, keys_per_s=S * E / r["median_ms"] * 1e3,
                         delivery_sweep_ms=d["ms_per_sweep"], delivery_sweep_median_ms=d["median_ms"],
                         ratio_to_delivery_sweep=r["median_ms"] / d["median_ms"])
                out[f"seeds_{S}_E{E}_{r['mode']}"] = r
                print(f"S={S} E={E} {r['mode']}: target + top-{K} {r['median_ms']:.3f} ms  delivery "
                      f"{d['median_ms']:.3f} ms  ratio {r['ratio_to_delivery_sweep']:.2f}  "
                      f"{r['keys_per_s']:.4g} keys/s  spread {r['spread']:.2%}", flush=True)
                _lib.check(L.nmz_replayable_target_plan_destroy(tplan))
                _lib.check(L.nmz_replayable_delivery_plan_destroy(dplan))
    return out


def inversions_rows(v, bits):
    """Per row of v (permutations of 0 .. 2^bits - 1): pairs i < j with v[i] > v[j]. Bit by bit from the top: rows
    stay grouped by the higher bits, a pair whose first differing bit is b is an inversion iff the 1 comes first."""
    inv = np.zeros(len(v), np.int64)
    cur = v
    for b in reversed(range(bits)):
        bit = (cur >> b) & 1
        cs = np.cumsum(bit, axis=1) - bit  # ones before, over the row
        g = 1 << (b + 1)
        ones_before = cs - np.repeat(cs[:, ::g], g, axis=1)
        inv += (ones_before * (1 - bit)).sum(axis=1)
        cur = np.take_along_axis(cur, np.argsort(cur >> b, axis=1, kind="stable"), axis=1)
    return inv


def host_route(a, L, ctx):
    """2^16 seeds x 1,024 events, exact mode, to a host top-64 by (n_discordant asc, seed asc)."""
    S, E = a.gate_seeds, a.gate_events
    bits = E.bit_length() - 1
    assert 1 << bits == E, "the numpy inversion count takes a power of two"
    hints, arrival, sym, _ = trace(E, False)
    hoff, hb = to_csr(hints)
    tp = recorded_target(L, hoff, hb, E, arrival, sym, None)
    soff, sb = to_csr([str(i) for i in range(S)])
    delays = np.zeros((S, E), np.int64)
    parts = {}

    def old():
        t0 = time.perf_counter()
        _lib.check(L.nmz_replayable_sweep(ctx.handle, p(soff), p(sb), S, p(hoff), p(hb), E, M, None, p(delays), S, 0,
                                          None))
        t1 = time.perf_counter()
        nd = np.zeros(S, np.int64)
        t_sort = 0.0
        for lo in range(0, S, 4096):  # row blocks keep the temporaries in cache-sized pieces
            t2 = time.perf_counter()
            order = np.argsort(delays[lo:lo + 4096] + arrival[None, :], axis=1, kind="stable")  # ties by index
            t_sort += time.perf_counter() - t2
            nd[lo:lo + 4096] = inversions_rows(tp[order].astype(np.int32), bits)
        t3 = time.perf_counter()
        parts.setdefault("dump_ms", []).append((t1 - t0) * 1e3)
        parts.setdefault("argsort_ms", []).append(t_sort * 1e3)
        parts.setdefault("inversion_count_ms", []).append((t3 - t1 - t_sort) * 1e3)
        return nd

    def new():
        st = np.zeros(S, _lib.TARGET_STATS_DTYPE)
        tk = np.zeros(K, _lib.TOPK_DTYPE)
        _lib.check(L.nmz_replayable_target_sweep_decimal(ctx.handle, 0, S, p(hoff), p(hb), E, M, p(arrival), None, p(tp),
                                                         0, K, p(st), p(tk), None, None))
        return st, tk

    new()  # warm-up: code objects
    t_old, t_new = [], []
    for _ in range(a.gate_reps):
        t0 = time.perf_counter()
        nd = old()
        t1 = time.perf_counter()
        st, _tk = new()
        t2 = time.perf_counter()
        t_old.append((t1 - t0) * 1e3)
        t_new.append((t2 - t1) * 1e3)
        assert np.array_equal(nd, st["n_discordant"]), "the two routes disagree"
    mo, mn = float(np.median(t_old)), float(np.median(t_new))
    print(f"host route {mo:.1f} ms, target sweep {mn:.2f} ms, ratio {mo / mn:.1f}x", flush=True)
    return {"seeds": S, "events": E, "delay_bytes_to_host": S * E * 8, "host_route_ms": t_old,
            "host_route_parts_ms": parts, "target_sweep_ms": t_new, "host_route_median_ms": mo,
            "target_sweep_median_ms": mn, "ratio": mo / mn, "results_equal": True,
            "what": "end to end from host arrays to host n_discordant[n_seeds], each call creating its own plan; host "
                    "route = nmz_replayable_sweep(n_dump_seeds = n_seeds) + numpy stable argsort + numpy inversion "
                    "count, new = nmz_replayable_target_sweep_decimal(stats + top-64)"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", type=int, nargs="+", default=[1 << 16, 1 << 20])
    ap.add_argument("--events", type=int, nargs="+", default=[64, 1024, 4096])
    ap.add_argument("--gate-seeds", type=int, default=1 << 16)
    ap.add_argument("--gate-events", type=int, default=1024)
    ap.add_argument("--gate-reps", type=int, default=1)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.25)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "target", "rate.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("target_rate.py measures on the GPU; no device found")
    L = _lib.load()
    ctx = _lib.Context(0)
    record = {"workload": {"hints": "configs[1] table (bench.py zk_hints)", "max_interval_ns": M,
                           "arrival_spacing_ns": 25_000, "po_entities": N_ENT, "top_k": K, "windows": a.reps,
                           "window_seconds": a.window, "target": "the delivery order of seed 'recorded-run'"},
              "timing": "host clock around back-to-back sweeps on one stream, each window ended by a synchronise; "
                        "profiler off",
              "sweep_and_topk": rate_configs(a, L, ctx, torch),
              "host_route": host_route(a, L, ctx)}
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(record, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
