"""Edit-script rate (a tool, not a bench leg): nmz_ed_align_pairs_dev over stores from the generator of the
bench's configs[2] clustered leg (namazu_amd/synth.clustered_traces, families of 1,024 near-duplicate runs), the pairs
being each trace with its nearest neighbour from nmz_ed_allpairs_knn -- the question a k-NN search leaves open.

Measured, profiler off:
  * shapes (trace length, band) = (2,048, 32), (2,048, 64), (256, 8) x 4,096 and 65,536 pairs (a store of as many
    traces), and one variant of (2,048, 32) with every second pair re-aimed at another family (beyond the band: the
    length filter does not catch it, the cut-off does): a few warm-up calls, then `--reps` windows of back-to-back
    calls on one stream through one plan, each window ended by a synchronise and sized to about `--window` seconds
    (host clock). Reported: the median ms per call, its spread, pairs/s. Before the timing the first pairs of the
    device result are compared with nmz_ed_align_host.
  * beside it, in the same run, host arrays to host arrays over the same pairs: nmz_ed_pairs (the distance-only
    route: the ratio is what history and walk cost) against nmz_ed_align_pairs, alternating, equal distances
    asserted; and, at 4,096 pairs, nmz_ed_align_host on 16 Python threads (ctypes drops the GIL) -- the only other
    route to a script -- with equal results asserted slot for slot. Both ratios are recorded, not gated.
usage: python3 tools/align_rate.py [--out profiles/align/rate.json]
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

CHECK_PAIRS = 64
HOST_THREADS = 16
SHAPES = [(2048, 32, False), (2048, 64, False), (256, 8, False), (2048, 32, True)]


def host_scripts(ts, pairs, band, threads):
    """(dist, ops) of nmz_ed_align_host over the pairs, `threads` Python threads."""
    L = _lib.load()
    dist = np.zeros(len(pairs), np.uint32)
    ops = np.zeros((len(pairs), band), _lib.EDIT_OP_DTYPE)
    sym, off = ts.sym, ts.off.astype(np.int64)
    base, dbase, obase = sym.ctypes.data, dist.ctypes.data, ops.ctypes.data

    def chunk(lo, hi):
        for p in range(lo, hi):
            i, j = int(pairs[p, 0]), int(pairs[p, 1])
            rc = L.nmz_ed_align_host(ctypes.c_void_p(base + 8 * int(off[i])), int(off[i + 1] - off[i]),
                                     ctypes.c_void_p(base + 8 * int(off[j])), int(off[j + 1] - off[j]), band,
                                     ctypes.c_void_p(dbase + 4 * p), ctypes.c_void_p(obase + 12 * band * p))
            assert rc == 0
    step = max(1, len(pairs) // (threads * 8))
    with ThreadPoolExecutor(threads) as ex:
        list(ex.map(lambda lo: chunk(lo, min(lo + step, len(pairs))), range(0, len(pairs), step)))
    return dist, ops


def nearest_pairs(ts, band, half_far, family, ctx):
    ids, _ = hs.allpairs_knn(ts, 1, band, ctx=ctx)
    n = len(ts)
    nb = np.where(ids[:, 0] == _lib.NMZ_NONE, (np.arange(n) + 1) % n, ids[:, 0]).astype(np.uint32)
    if half_far:
        nb[1::2] = ((np.arange(n) + family) % n).astype(np.uint32)[1::2]
    return np.stack([np.arange(n, dtype=np.uint32), nb], 1)


def one(a, length, band, half_far, P, ctx, torch, stream):
    family = min(1024, P // 4)
    ts = synth.clustered_traces(P, length, family=family)
    pairs = nearest_pairs(ts, band, half_far, family, ctx)
    plan = hs.AlignPlan(band, int(np.diff(ts.off.astype(np.int64)).max()), ctx=ctx)
    d_off = torch.from_numpy(ts.off.view(np.int64)).cuda()
    d_sym = torch.from_numpy(ts.sym.view(np.int64)).cuda()
    d_pairs = torch.from_numpy(pairs.view(np.int32)).cuda()
    d_dist = torch.zeros(P, dtype=torch.int32, device="cuda")
    d_ops = torch.zeros(P * band * 3, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()

    def step():
        plan.pairs_dev(d_off.data_ptr(), d_sym.data_ptr(), d_pairs.data_ptr(), P, d_dist.data_ptr(), d_ops.data_ptr(),
                       stream.cuda_stream)

    step()
    stream.synchronize()
    dist = d_dist.cpu().numpy().view(np.uint32)
    ops = d_ops.cpu().numpy().view(_lib.EDIT_OP_DTYPE).reshape(P, band)
    hd, ho = host_scripts(ts, pairs[:CHECK_PAIRS], band, 1)
    assert np.array_equal(dist[:CHECK_PAIRS], hd) and ops[:CHECK_PAIRS].tobytes() == ho.tobytes(), "scripts are wrong"
    m = windows(step, stream.synchronize, a.warmup, a.reps, a.window)
    r = {"length": length, "band": band, "pairs": P, "half_beyond_band": half_far, "slots": plan.slots,
         "history_bytes": plan.history_bytes, "in_band_fraction": float((dist <= band).mean()),
         "mean_script_ops": float(dist[dist <= band].mean()) if (dist <= band).any() else 0.0, "align_dev": m,
         "pairs_per_s": P / m["median_ms"] * 1e3, "pairs_checked": CHECK_PAIRS}
    plan.close()
    del d_off, d_sym, d_pairs, d_dist, d_ops
    # host arrays to host arrays: the distance-only route beside the scripts
    t_ed, t_al = [], []
    for f in (lambda: hs.ed_pairs(ts, pairs, band, ctx=ctx), lambda: hs.edit_scripts(ts, pairs, band, ctx=ctx)):
        f()
    for _ in range(a.reps):
        t0 = time.perf_counter()
        de = hs.ed_pairs(ts, pairs, band, ctx=ctx)
        t1 = time.perf_counter()
        es = hs.edit_scripts(ts, pairs, band, ctx=ctx)
        t2 = time.perf_counter()
        t_ed.append((t1 - t0) * 1e3)
        t_al.append((t2 - t1) * 1e3)
        assert np.array_equal(de, es.dist) and np.array_equal(es.dist, dist), "the two routes disagree"
    r["host_arrays"] = {"ed_pairs_ms": t_ed, "ed_align_pairs_ms": t_al, "ed_pairs_median_ms": float(np.median(t_ed)),
                        "ed_align_pairs_median_ms": float(np.median(t_al)),
                        "align_over_ed_pairs": float(np.median(t_al) / np.median(t_ed)), "distances_equal": True}
    line = (f"L={length} w={band} P={P}{' half-far' if half_far else ''}: dev {m['median_ms']:.3f} ms/call (spread "
            f"{m['spread']:.2%}, {r['pairs_per_s']:.4g} pairs/s, {plan.slots} slots)  host arrays: ed_pairs "
            f"{np.median(t_ed):.2f} ms, ed_align_pairs {np.median(t_al):.2f} ms")
    if P <= a.host_pairs:
        t_h = []
        for _ in range(max(1, a.reps // 2)):
            t0 = time.perf_counter()
            hd, ho = host_scripts(ts, pairs, band, HOST_THREADS)
            t_h.append((time.perf_counter() - t0) * 1e3)
        assert np.array_equal(hd, dist) and ho.tobytes() == ops.tobytes(), "host threads and device disagree"
        r["host_threads"] = {"threads": HOST_THREADS, "ms": t_h, "median_ms": float(np.median(t_h)),
                             "over_ed_align_pairs": float(np.median(t_h) / np.median(t_al)),
                             "over_align_dev": float(np.median(t_h) / m["median_ms"]), "results_equal": True}
        ratio = r["host_threads"]["over_ed_align_pairs"]
        line += f", {HOST_THREADS} host threads {np.median(t_h):.1f} ms ({ratio:.1f}x)"
    print(line, flush=True)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, nargs="+", default=[4096, 65536])
    ap.add_argument("--host-pairs", type=int, default=4096, help="largest pair count the 16 host threads run")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.25)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "align", "rate.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("align_rate.py measures on the GPU; no device found")
    ctx = _lib.Context(0)
    stream = torch.cuda.Stream()
    shapes = {}
    for length, band, half_far in SHAPES:
        for P in a.pairs:
            key = f"L{length}_w{band}_P{P}" + ("_halffar" if half_far else "")
            shapes[key] = one(a, length, band, half_far, P, ctx, torch, stream)
    record = {"workload": {"generator": "namazu_amd/synth.clustered_traces (the bench's configs[2] clustered leg)",
                           "pairs": "each trace with its nearest neighbour (nmz_ed_allpairs_knn, k = 1)",
                           "warmup_calls": a.warmup, "windows": a.reps, "window_seconds": a.window},
              "timing": "host clock around back-to-back calls on one stream, each window ended by a synchronise; "
                        "profiler off",
              "shapes": shapes}
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(record, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
