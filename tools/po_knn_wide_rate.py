"""PO k-NN search rate over bands 65 .. 1,024 (a tool, not a bench leg): K11w (k_po_knn_wide) over tools/po_knn_rate.py's
workload -- a resident clustered store of 2,048-event traces with 16 entities (namazu_amd/synth.clustered_traces; a
symbol's entity is its rank among the store's symbols mod 16), the queries members of the store spread over its
families, each skipping itself, k = 8.

Measured, profiler off, the compared forms' windows alternating, every window's figure kept:
  * host arrays to host arrays, 64 queries x the 4,096-trace store at bands 128 and 512: nmz_po_knn_wide against the
    only earlier route at these bands -- all 262,144 pairs through nmz_ed_align_po_pairs, then lexsort. Lists must
    be equal (asserted);
  * the step from 64 to 65: one wide plan type at band 64 (it runs k_po_knn<3>) and at band 65 (k_po_knn_wide<1>),
    1 / 64 / 1,024 queries, the device form;
  * the clamp's worth: the default against NMZ_PO_KNN_OPT_FULL_BAND at bands 128, 512 and 1,024 (equal lists
    asserted), the device form, with the per-C entity-step counters, the filter's share of the pairs and the resident
    bytes beside the times.
Ratios are recorded, not gated.
usage: python3 tools/po_knn_wide_rate.py [--out profiles/po_knn_wide/rate.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
from namazu_amd import _lib, historystorage as hs, synth  # noqa: E402
from po_knn_rate import earlier_route  # noqa: E402

LENGTH = 2048
ENTITIES = 16
K = 8


def window(step, sync, seconds):
    """ms per call over one window of back-to-back calls (at least one), ended by a synchronise."""
    t0 = time.perf_counter()
    n = 0
    while n == 0 or time.perf_counter() - t0 < seconds:
        step()
        n += 1
        if n == 1:
            sync()  # the first call's time sizes the window
    sync()
    return (time.perf_counter() - t0) / n * 1e3, n


def fold(ms):
    v = [m for m, _ in ms]
    med = float(np.median(v))
    return {"ms_per_call": v, "median_ms": med, "min_ms": min(v), "max_ms": max(v), "spread": (max(v) - min(v)) / med,
            "calls_per_window": [n for _, n in ms]}


class Queries:
    """Q members of the store on the device, for the _dev form."""

    def __init__(self, torch, ts, ent, Q):
        N = len(ts)
        self.Q = Q
        self.members = (np.arange(Q, dtype=np.int64) * N // Q).astype(np.uint32)  # spread over the families
        self.qts = hs.TraceSet([ts.trace(int(m)) for m in self.members])
        self.q_ent = np.concatenate([ent[int(ts.off[m]):int(ts.off[m + 1])] for m in self.members])
        self.elems = int(self.qts.off[-1])
        self.d_off = torch.from_numpy(self.qts.off.view(np.int64)).cuda()
        self.d_sym = torch.from_numpy(self.qts.sym.view(np.int64)).cuda()
        self.d_ent = torch.from_numpy(np.ascontiguousarray(self.q_ent).view(np.int32)).cuda()
        self.d_self = torch.from_numpy(self.members.view(np.int32)).cuda()
        self.d_keys = torch.zeros(Q * K, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()

    def step(self, plan, stream):
        plan.query_dev(self.d_off.data_ptr(), self.d_sym.data_ptr(), self.d_ent.data_ptr(), self.d_self.data_ptr(),
                       self.Q, K, self.d_keys.data_ptr(), stream.cuda_stream)


def compare_dev(a, torch, ctx, stream, ts, ent, q, forms):
    """forms: {name: (band, opts)}. One wide plan each; a first call each for the lists and the counters, then
    a.reps rounds of one window per form, alternating."""
    plans = {name: hs.PoSimilarityIndex(ts, ent, band, ctx=ctx, n_entities=ENTITIES, max_queries=q.Q,
                                        max_query_elems=q.elems, opts=opts, wide=True)
             for name, (band, opts) in forms.items()}
    out, keys, ms = {}, {}, {name: [] for name in forms}
    for name, plan in plans.items():
        q.step(plan, stream)
        stream.synchronize()
        keys[name] = q.d_keys.cpu().numpy().copy()
        c = plan.counters(stream.cuda_stream)
        resident, blocks, waves = plan.info()
        eligible = q.Q * (len(ts) - 1)
        out[name] = {"band": forms[name][0], "opts": forms[name][1], "counters": c, "resident_bytes": resident,
                     "workgroups": blocks, "waves": waves, "filtered_share": c["filtered"] / eligible,
                     "dp_share": c["dp"] / eligible, "in_band_share": c["in_band"] / eligible}
    for _ in range(a.reps):
        for name, plan in plans.items():
            ms[name].append(window(lambda: q.step(plan, stream), stream.synchronize, a.window))
    for name, plan in plans.items():
        out[name]["dev"] = fold(ms[name])
        plan.close()
    return out, keys


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--store", type=int, default=4096)
    ap.add_argument("--step-queries", type=int, nargs="*", default=[1, 64, 1024])
    ap.add_argument("--clamp-queries", type=int, default=64)
    ap.add_argument("--clamp-bands", type=int, nargs="*", default=[128, 512, 1024])
    ap.add_argument("--host-bands", type=int, nargs="*", default=[128, 512])
    ap.add_argument("--host-queries", type=int, default=64)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--window", type=float, default=0.25)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "po_knn_wide", "rate.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("po_knn_wide_rate.py measures on the GPU; no device found")
    ctx = _lib.Context(0)
    stream = torch.cuda.Stream()
    N, G = a.store, ENTITIES
    ts = synth.clustered_traces(N, LENGTH, family=min(1024, N // 4))
    total = int(ts.off[-1])
    ent = (np.searchsorted(np.unique(ts.sym[:total]), ts.sym[:total]) % G).astype(np.uint32)
    record = {"workload": {"generator": "namazu_amd/synth.clustered_traces (the bench's configs[2] clustered leg)",
                           "length": LENGTH, "store": N, "k": K,
                           "entities": "a symbol's rank among the store's symbols mod 16",
                           "queries": "members of the store spread evenly over its families, each skipping itself",
                           "windows": a.reps, "window_seconds": a.window},
              "timing": "host clock around back-to-back calls on one stream, each window ended by a synchronise (at "
                        "least one call per window); the compared forms' windows alternate; profiler off.",
              "step_64_65": {}, "clamp": {}, "host_arrays": {}}

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(record, f, indent=1, sort_keys=True)
            f.write("\n")

    # ---- the step from 64 to 65
    for Q in a.step_queries:
        q = Queries(torch, ts, ent, Q)
        r, _ = compare_dev(a, torch, ctx, stream, ts, ent, q, {"w64_k_po_knn": (64, 0), "w65_k_po_knn_wide": (65, 0)})
        r["w65_over_w64"] = r["w65_k_po_knn_wide"]["dev"]["median_ms"] / r["w64_k_po_knn"]["dev"]["median_ms"]
        record["step_64_65"][f"Q{Q}"] = r
        print(f"step Q={Q}: w=64 {r['w64_k_po_knn']['dev']['median_ms']:.3f} ms/call (spread "
              f"{r['w64_k_po_knn']['dev']['spread']:.2%}), w=65 {r['w65_k_po_knn_wide']['dev']['median_ms']:.3f} ms/call "
              f"(spread {r['w65_k_po_knn_wide']['dev']['spread']:.2%})", flush=True)
        save()
    # ---- the clamp's worth
    q = Queries(torch, ts, ent, a.clamp_queries)
    for band in a.clamp_bands:
        r, keys = compare_dev(a, torch, ctx, stream, ts, ent, q,
                              {"clamped": (band, 0), "full_band": (band, _lib.NMZ_PO_KNN_OPT_FULL_BAND)})
        assert np.array_equal(keys["clamped"], keys["full_band"]), "the clamp changed a list"
        r["full_band_over_clamped"] = r["full_band"]["dev"]["median_ms"] / r["clamped"]["dev"]["median_ms"]
        record["clamp"][f"w{band}_Q{a.clamp_queries}"] = r
        c = r["clamped"]
        print(f"clamp w={band} Q={a.clamp_queries}: clamped {c['dev']['median_ms']:.3f} ms/call (spread "
              f"{c['dev']['spread']:.2%}), full band {r['full_band']['dev']['median_ms']:.3f} ms/call (spread "
              f"{r['full_band']['dev']['spread']:.2%}); filtered {c['filtered_share']:.2%}, DP {c['dp_share']:.2%}, in "
              f"band {c['in_band_share']:.2%}; steps {[c['counters'][s] for s in hs.PoSimilarityIndex.STEP_NAMES]} / "
              f"{[r['full_band']['counters'][s] for s in hs.PoSimilarityIndex.STEP_NAMES]}; resident "
              f"{c['resident_bytes']} bytes", flush=True)
        save()
    # ---- host arrays to host arrays against the only earlier route
    q = Queries(torch, ts, ent, a.host_queries)
    for band in a.host_bands:
        t_new, t_old = [], []
        for _ in range(a.host_reps):
            t0 = time.perf_counter()
            ids, ds = hs.po_knn_wide(ts, ent, q.qts, q.q_ent, K, band, n_entities=G, q_self=q.members, ctx=ctx)
            t1 = time.perf_counter()
            oi, od, script_bytes = earlier_route(ts, ent, G, q.members.tolist(), band, K, ctx)
            t2 = time.perf_counter()
            t_new.append((t1 - t0) * 1e3)
            t_old.append((t2 - t1) * 1e3)
            assert np.array_equal(ids, oi) and np.array_equal(ds, od), "K11w and the pairwise route disagree"
            print(f"host arrays, w={band} Q={q.Q} N={N}: nmz_po_knn_wide {t_new[-1]:.1f} ms, all pairs through "
                  f"nmz_ed_align_po_pairs + lexsort {t_old[-1]:.1f} ms", flush=True)
        record["host_arrays"][f"w{band}"] = {
            "band": band, "queries": q.Q, "store": N, "pairs": q.Q * N, "po_knn_wide_ms": t_new,
            "pairwise_route_ms": t_old, "po_knn_wide_median_ms": float(np.median(t_new)),
            "pairwise_route_median_ms": float(np.median(t_old)),
            "po_knn_wide_range_ms": [min(t_new), max(t_new)], "pairwise_route_range_ms": [min(t_old), max(t_old)],
            "ranges_overlap": not (max(t_new) < min(t_old) or max(t_old) < min(t_new)),
            "pairwise_route_over_po_knn_wide": float(np.median(t_old) / np.median(t_new)),
            "pairwise_route_script_bytes": script_bytes, "lists_equal": True}
        save()
    ctx.close()


if __name__ == "__main__":
    main()
