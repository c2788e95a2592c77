"""Wide edit-script rate (a tool, not a bench leg): nmz_ed_align_wide_pairs_dev, bands beyond 64, over stores from
the generator of the bench's configs[2] clustered leg (namazu_amd/synth.clustered_traces), the pairs being each trace
with its nearest neighbour at the band from nmz_ed_allpairs_knn -- tools/align_rate.py's pattern one level up.

Measured, profiler off:
  * traces of 2,048 elements at bands 65, 128, 512 and 1,024 (C = 1, 2, 5, 9 cells per thread) x 256 and 4,096
    pairs (a store of as many traces), and at 4,096 pairs a variant whose partner is the trace itself with its
    first band / 4 elements moved to the end (scripts of about band / 2 ops: what a long walk costs; the store's
    own neighbours are a few edits apart): a few warm-up calls, then `--reps` windows of back-to-back calls on one
    stream through one plan, each window ended by a synchronise and sized to about `--window` seconds (host
    clock). Reported: the median ms per call, its spread, pairs/s. Every pair of the device result is
    compared with the host form (below).
  * beside it, in the same run, over the same pairs, alternating window for window: the narrow
    nmz_ed_align_pairs_dev at band 64 -- the yardstick for the step from 64 to 65 (the stores' neighbours are a
    few edits apart, so both give the same scripts: asserted);
  * host arrays to host arrays, alternating: nmz_ed_pairs (the distance-only route) against
    nmz_ed_align_wide_pairs, equal distances asserted;
  * nmz_ed_align_wide_host on 16 Python threads (ctypes drops the GIL), the only other route to a wide script,
    equal slot for slot (asserted).
Ratios are recorded, not gated.
usage: python3 tools/align_wide_rate.py [--out profiles/align_wide/rate.json]
"""
import argparse
import ctypes
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
from namazu_amd import _lib, historystorage as hs, synth  # noqa: E402
from order_rate import windows  # noqa: E402

HOST_THREADS = 16
LENGTH = 2048
BANDS = [65, 128, 512, 1024]
NARROW = _lib.NMZ_ALIGN_MAX_BAND


def host_scripts(ts, pairs, band, threads):
    """(dist, ops) of nmz_ed_align_wide_host over the pairs, `threads` Python threads."""
    L = _lib.load()
    dist = np.zeros(len(pairs), np.uint32)
    ops = np.zeros((len(pairs), band), _lib.EDIT_OP_DTYPE)
    sym, off = ts.sym, ts.off.astype(np.int64)
    base, dbase, obase = sym.ctypes.data, dist.ctypes.data, ops.ctypes.data

    def chunk(lo, hi):
        for p in range(lo, hi):
            i, j = int(pairs[p, 0]), int(pairs[p, 1])
            rc = L.nmz_ed_align_wide_host(ctypes.c_void_p(base + 8 * int(off[i])), int(off[i + 1] - off[i]),
                                          ctypes.c_void_p(base + 8 * int(off[j])), int(off[j + 1] - off[j]), band,
                                          ctypes.c_void_p(dbase + 4 * p), ctypes.c_void_p(obase + 12 * band * p))
            assert rc == 0
    step = max(1, len(pairs) // (threads * 8))
    with ThreadPoolExecutor(threads) as ex:
        list(ex.map(lambda lo: chunk(lo, min(lo + step, len(pairs))), range(0, len(pairs), step)))
    return dist, ops


def nearest_pairs(ts, band, ctx):
    ids, _ = hs.allpairs_knn(ts, 1, band, ctx=ctx)
    n = len(ts)
    nb = np.where(ids[:, 0] == _lib.NMZ_NONE, (np.arange(n) + 1) % n, ids[:, 0]).astype(np.uint32)
    return np.stack([np.arange(n, dtype=np.uint32), nb], 1)


def one(a, band, P, far, ctx, torch, stream):
    ts = synth.clustered_traces(P, LENGTH, family=min(1024, P // 4))
    if far:  # every trace against itself with its first band / 4 elements moved to the end: about band / 2 edits
        trs = [ts.trace(i) for i in range(P)]
        ts = hs.TraceSet(trs + [np.concatenate([t[band // 4:], t[:band // 4]]) for t in trs])
        pairs = np.stack([np.arange(P, dtype=np.uint32), np.arange(P, 2 * P, dtype=np.uint32)], 1)
    else:
        pairs = nearest_pairs(ts, band, ctx)
    max_len = int(np.diff(ts.off.astype(np.int64)).max())
    plan, narrow = hs.AlignWidePlan(band, max_len, ctx=ctx), hs.AlignPlan(NARROW, max_len, ctx=ctx)
    d_off = torch.from_numpy(ts.off.view(np.int64)).cuda()
    d_sym = torch.from_numpy(ts.sym.view(np.int64)).cuda()
    d_pairs = torch.from_numpy(pairs.view(np.int32)).cuda()
    d_dist = torch.zeros(P, dtype=torch.int32, device="cuda")
    d_ops = torch.zeros(P * band * 3, dtype=torch.int32, device="cuda")
    n_dist = torch.zeros(P, dtype=torch.int32, device="cuda")
    n_ops = torch.zeros(P * NARROW * 3, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()

    def step():
        plan.pairs_dev(d_off.data_ptr(), d_sym.data_ptr(), d_pairs.data_ptr(), P, d_dist.data_ptr(), d_ops.data_ptr(),
                       stream.cuda_stream)

    def step_narrow():
        narrow.pairs_dev(d_off.data_ptr(), d_sym.data_ptr(), d_pairs.data_ptr(), P, n_dist.data_ptr(),
                         n_ops.data_ptr(), stream.cuda_stream)

    step()
    step_narrow()
    stream.synchronize()
    dist = d_dist.cpu().numpy().view(np.uint32)
    ops = d_ops.cpu().numpy().view(_lib.EDIT_OP_DTYPE).reshape(P, band)
    nd = n_dist.cpu().numpy().view(np.uint32)
    no = n_ops.cpu().numpy().view(_lib.EDIT_OP_DTYPE).reshape(P, NARROW)
    near = nd <= NARROW
    assert np.array_equal(dist[near], nd[near]) and ops[near, :NARROW].tobytes() == no[near].tobytes(), \
        "the wide and the narrow kernel disagree within 64 edits"
    # alternating, one window each per round, so that both see the same machine
    m_w, m_n = [], []
    for r in range(a.reps):
        m_w.append(windows(step, stream.synchronize, a.warmup if r == 0 else 1, 1, a.window))
        m_n.append(windows(step_narrow, stream.synchronize, a.warmup if r == 0 else 1, 1, a.window))

    def fold(ms):
        v = [x["median_ms"] for x in ms]
        med = float(np.median(v))
        return {"ms_per_call": v, "median_ms": med, "spread": (max(v) - min(v)) / med,
                "calls_per_window": [x["sweeps_per_window"] for x in ms]}

    m, mn = fold(m_w), fold(m_n)
    r = {"length": LENGTH, "band": band, "pairs": P, "rotated_partner": far, "slots": plan.slots,
         "history_bytes": plan.history_bytes,
         "in_band_fraction": float((dist <= band).mean()),
         "mean_script_ops": float(dist[dist <= band].mean()) if (dist <= band).any() else 0.0,
         "max_script_ops": int(dist[dist <= band].max()) if (dist <= band).any() else 0,
         "align_wide_dev": m, "pairs_per_s": P / m["median_ms"] * 1e3,
         "narrow_w64_dev": dict(mn, slots=narrow.slots, pairs_per_s=P / mn["median_ms"] * 1e3,
                                within_64_fraction=float(near.mean())),
         "wide_over_narrow_w64": m["median_ms"] / mn["median_ms"]}
    plan.close()
    narrow.close()
    del d_off, d_sym, d_pairs, d_dist, d_ops, n_dist, n_ops
    # host arrays to host arrays: the distance-only route beside the scripts
    t_ed, t_al = [], []
    for f in (lambda: hs.ed_pairs(ts, pairs, band, ctx=ctx), lambda: hs.edit_scripts_wide(ts, pairs, band, ctx=ctx)):
        f()
    for _ in range(a.reps):
        t0 = time.perf_counter()
        de = hs.ed_pairs(ts, pairs, band, ctx=ctx)
        t1 = time.perf_counter()
        es = hs.edit_scripts_wide(ts, pairs, band, ctx=ctx)
        t2 = time.perf_counter()
        t_ed.append((t1 - t0) * 1e3)
        t_al.append((t2 - t1) * 1e3)
        assert np.array_equal(de, es.dist) and np.array_equal(es.dist, dist), "the two routes disagree"
        assert es.ops.tobytes() == ops.tobytes(), "the host-pointer and the device-pointer form disagree"
    r["host_arrays"] = {"ed_pairs_ms": t_ed, "ed_align_wide_pairs_ms": t_al,
                        "ed_pairs_median_ms": float(np.median(t_ed)),
                        "ed_align_wide_pairs_median_ms": float(np.median(t_al)),
                        "align_over_ed_pairs": float(np.median(t_al) / np.median(t_ed)), "distances_equal": True}
    t_h = []
    for _ in range(a.host_reps):
        t0 = time.perf_counter()
        hd, ho = host_scripts(ts, pairs, band, HOST_THREADS)
        t_h.append((time.perf_counter() - t0) * 1e3)
    assert np.array_equal(hd, dist) and ho.tobytes() == ops.tobytes(), "host threads and device disagree"
    r["host_threads"] = {"threads": HOST_THREADS, "ms": t_h, "median_ms": float(np.median(t_h)),
                         "over_ed_align_wide_pairs": float(np.median(t_h) / np.median(t_al)),
                         "over_align_wide_dev": float(np.median(t_h) / m["median_ms"]), "results_equal": True,
                         "pairs_checked": P}
    print(f"L={LENGTH} w={band} P={P}{' rotated' if far else ''}: wide dev {m['median_ms']:.3f} ms/call (spread {m['spread']:.2%}, "
          f"{r['pairs_per_s']:.4g} pairs/s, {r['slots']} slots, max script {r['max_script_ops']})  narrow w=64 dev "
          f"{mn['median_ms']:.3f} ms/call  host arrays: ed_pairs {np.median(t_ed):.2f} ms, ed_align_wide_pairs "
          f"{np.median(t_al):.2f} ms  {HOST_THREADS} host threads {np.median(t_h):.1f} ms", flush=True)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, nargs="+", default=[256, 4096])
    ap.add_argument("--bands", type=int, nargs="+", default=BANDS)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-reps", type=int, default=1)
    ap.add_argument("--window", type=float, default=0.25)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "align_wide", "rate.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("align_wide_rate.py measures on the GPU; no device found")
    ctx = _lib.Context(0)
    stream = torch.cuda.Stream()
    shapes = {}
    for band in a.bands:
        for P in a.pairs:
            shapes[f"L{LENGTH}_w{band}_P{P}"] = one(a, band, P, False, ctx, torch, stream)
        P = max(a.pairs)
        shapes[f"L{LENGTH}_w{band}_P{P}_rotated"] = one(a, band, P, True, ctx, torch, stream)
    record = {"workload": {"generator": "namazu_amd/synth.clustered_traces (the bench's configs[2] clustered leg)",
                           "pairs": "each trace with its nearest neighbour at the band (nmz_ed_allpairs_knn, k = 1)",
                           "warmup_calls": a.warmup, "windows": a.reps, "window_seconds": a.window},
              "timing": "host clock around back-to-back calls on one stream, each window ended by a synchronise; the "
                        "wide plan's windows alternate with the narrow plan's; profiler off",
              "shapes": shapes}
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(record, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
