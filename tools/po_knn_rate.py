"""PO k-NN search rate (a tool, not a bench leg): nmz_po_knn_query_dev over a resident clustered store of 2,048-event
traces with 16 entities (the generator of the bench's configs[2] clustered leg, namazu_amd/synth.clustered_traces; a
symbol's entity is its rank among the store's symbols mod 16, so a symbol determines its entity as an event does) --
tools/align_po_rate.py's pattern.

Measured, profiler off:
  * 1, 64 and 1,024 queries (members of the store, each skipping itself) against the 4,096-trace store at bands 8,
    32 and 64: ms per call of the device form with the four counters, and beside it in the same run, alternating
    window for window, nmz_ed_plan_query_knn (the exact search) over the same store and queries, K11 under
    NMZ_PO_KNN_OPT_NO_FILTER and K11 under NMZ_PO_KNN_OPT_WHOLE_BLOCKS (equal lists asserted);
  * 64 queries x 4,096 stored traces at band 32, host arrays to host arrays: nmz_po_knn against the only earlier
    route -- all 262,144 pairs through nmz_ed_align_po_pairs, then lexsort. Lists must be equal (asserted).
Ratios are recorded, not gated.
usage: python3 tools/po_knn_rate.py [--out profiles/po_knn/rate.json]
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
from order_rate import windows  # noqa: E402

LENGTH = 2048
ENTITIES = 16
BANDS = [8, 32, 64]
QUERIES = [1, 64, 1024]
K = 8


def fold(ms):
    v = [x["median_ms"] for x in ms]
    med = float(np.median(v))
    return {"ms_per_call": v, "median_ms": med, "spread": (max(v) - min(v)) / med,
            "calls_per_window": [x["sweeps_per_window"] for x in ms]}


def earlier_route(ts, ent, G, members, band, k, ctx):
    """Every (query, stored trace) pair through nmz_ed_align_po_pairs, then lexsort: host arrays to host arrays."""
    N = len(ts)
    pairs = np.stack([np.repeat(np.asarray(members, np.uint32), N),
                      np.tile(np.arange(N, dtype=np.uint32), len(members))], 1)
    es = hs.edit_scripts_po(ts, ent, pairs, band, n_entities=G, ctx=ctx)
    D = es.dist.reshape(len(members), N)
    ids = np.full((len(members), k), _lib.NMZ_NONE, np.uint32)
    ds = np.full((len(members), k), _lib.NMZ_NONE, np.uint32)
    for r, m in enumerate(members):
        order = np.lexsort((np.arange(N), D[r]))
        order = order[order != m][:k]
        ids[r, :len(order)] = order
        ds[r, :len(order)] = D[r, order]
    return ids, ds, int(es.ops.nbytes)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--store", type=int, default=4096)
    ap.add_argument("--queries", type=int, nargs="+", default=QUERIES)
    ap.add_argument("--bands", type=int, nargs="+", default=BANDS)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--host-reps", type=int, default=2)
    ap.add_argument("--window", type=float, default=0.25)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "po_knn", "rate.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("po_knn_rate.py measures on the GPU; no device found")
    ctx = _lib.Context(0)
    stream = torch.cuda.Stream()
    N, G = a.store, ENTITIES
    ts = synth.clustered_traces(N, LENGTH, family=min(1024, N // 4))
    total = int(ts.off[-1])
    ent = (np.searchsorted(np.unique(ts.sym[:total]), ts.sym[:total]) % G).astype(np.uint32)
    shapes = {}
    for band in a.bands:
        for Q in a.queries:
            members = (np.arange(Q, dtype=np.int64) * N // Q).astype(np.uint32)  # spread over the families
            qts = hs.TraceSet([ts.trace(int(m)) for m in members])
            q_ent = np.concatenate([ent[int(ts.off[m]):int(ts.off[m + 1])] for m in members])
            q_elems = int(qts.off[-1])
            d_off = torch.from_numpy(qts.off.view(np.int64)).cuda()
            d_sym = torch.from_numpy(qts.sym.view(np.int64)).cuda()
            d_ent = torch.from_numpy(np.ascontiguousarray(q_ent).view(np.int32)).cuda()
            d_self = torch.from_numpy(members.view(np.int32)).cuda()
            d_keys = torch.zeros(Q * K, dtype=torch.int64, device="cuda")
            torch.cuda.synchronize()
            plans = {name: hs.PoSimilarityIndex(ts, ent, band, ctx=ctx, n_entities=G, max_queries=Q,
                                                max_query_elems=q_elems, opts=opts)
                     for name, opts in (("filter", 0), ("no_filter", _lib.NMZ_PO_KNN_OPT_NO_FILTER),
                                        ("whole_blocks", _lib.NMZ_PO_KNN_OPT_WHOLE_BLOCKS))}
            exact = hs.SimilarityIndex(ts, band, ctx=ctx)
            queries = [ts.trace(int(m)) for m in members]

            def step(name):
                plans[name].query_dev(d_off.data_ptr(), d_sym.data_ptr(), d_ent.data_ptr(), d_self.data_ptr(), Q, K,
                                      d_keys.data_ptr(), stream.cuda_stream)

            keys, counters = {}, {}
            for name in plans:
                step(name)
                stream.synchronize()
                keys[name] = d_keys.cpu().numpy().copy()
                counters[name] = plans[name].counters(stream.cuda_stream)
            assert np.array_equal(keys["filter"], keys["no_filter"]), "the filter changed a list"
            assert np.array_equal(keys["filter"], keys["whole_blocks"]), "the deal changed a list"
            assert counters["filter"] == counters["whole_blocks"], "the deal changed a counter"
            m_f, m_n, m_e, m_w = [], [], [], []
            for r in range(a.reps):  # alternating, one window each per round, so that all see the same machine
                wu = a.warmup if r == 0 else 1
                m_f.append(windows(lambda: step("filter"), stream.synchronize, wu, 1, a.window))
                m_n.append(windows(lambda: step("no_filter"), stream.synchronize, wu, 1, a.window))
                m_w.append(windows(lambda: step("whole_blocks"), stream.synchronize, wu, 1, a.window))
                m_e.append(windows(lambda: exact.query(queries, K), lambda: None, wu, 1, a.window))
            mf, mn, me, mw = fold(m_f), fold(m_n), fold(m_e), fold(m_w)
            c = counters["filter"]
            eligible = Q * (N - 1)
            resident, blocks, waves = plans["filter"].info()
            r = {"length": LENGTH, "band": band, "queries": Q, "store": N, "entities": G, "k": K,
                 "resident_bytes": resident, "blocks": blocks, "waves": waves, "counters": c,
                 "counters_no_filter": counters["no_filter"], "filtered_share": c["filtered"] / eligible,
                 "dp_share": c["dp"] / eligible, "in_band_share": c["in_band"] / eligible,
                 "po_knn_dev": mf, "pairs_per_s": eligible / mf["median_ms"] * 1e3,
                 "po_knn_no_filter_dev": mn, "po_knn_whole_blocks_dev": mw,
                 "whole_blocks_over_parts": mw["median_ms"] / mf["median_ms"],
                 # every in-band pair runs all of the query's rows; the rows of pairs cut off are not counted
                 "no_filter_dp_rows_per_s_lower_bound":
                     counters["no_filter"]["in_band"] * LENGTH / mn["median_ms"] * 1e3,
                 "ed_plan_query_knn_host_arrays": dict(me, kind=exact.kind),
                 "no_filter_over_filter": mn["median_ms"] / mf["median_ms"]}
            for p in plans.values():
                p.close()
            exact.close()
            shapes[f"L{LENGTH}_w{band}_Q{Q}_N{N}_G{G}"] = r
            print(f"w={band} Q={Q} N={N}: K11 {mf['median_ms']:.3f} ms/call (spread {mf['spread']:.2%}; filtered "
                  f"{r['filtered_share']:.2%}, DP {r['dp_share']:.2%}, in band {r['in_band_share']:.2%})  no filter "
                  f"{mn['median_ms']:.3f} ms/call  whole blocks {mw['median_ms']:.3f} ms/call  exact search "
                  f"{me['median_ms']:.3f} ms/call ({exact.kind})", flush=True)
    # host arrays to host arrays against the only earlier route
    band, Q = 32, 64
    members = (np.arange(Q, dtype=np.int64) * N // Q).astype(np.uint32)
    qts = hs.TraceSet([ts.trace(int(m)) for m in members])
    q_ent = np.concatenate([ent[int(ts.off[m]):int(ts.off[m + 1])] for m in members])
    t_new, t_old = [], []
    for _ in range(a.host_reps):
        t0 = time.perf_counter()
        ids, ds = hs.po_knn(ts, ent, qts, q_ent, K, band, n_entities=G, q_self=members, ctx=ctx)
        t1 = time.perf_counter()
        oi, od, script_bytes = earlier_route(ts, ent, G, members.tolist(), band, K, ctx)
        t2 = time.perf_counter()
        t_new.append((t1 - t0) * 1e3)
        t_old.append((t2 - t1) * 1e3)
        assert np.array_equal(ids, oi) and np.array_equal(ds, od), "K11 and the pairwise route disagree"
        print(f"host arrays, w={band} Q={Q} N={N}: nmz_po_knn {t_new[-1]:.1f} ms, all pairs through "
              f"nmz_ed_align_po_pairs + lexsort {t_old[-1]:.1f} ms", flush=True)

    def spread(v):
        return (max(v) - min(v)) / float(np.median(v))

    host = {"band": band, "queries": Q, "store": N, "pairs": Q * N, "po_knn_ms": t_new, "pairwise_route_ms": t_old,
            "po_knn_median_ms": float(np.median(t_new)), "pairwise_route_median_ms": float(np.median(t_old)),
            "po_knn_spread": spread(t_new), "pairwise_route_spread": spread(t_old),
            "pairwise_route_over_po_knn": float(np.median(t_old) / np.median(t_new)),
            "pairwise_route_script_bytes": script_bytes, "lists_equal": True}
    record = {"workload": {"generator": "namazu_amd/synth.clustered_traces (the bench's configs[2] clustered leg)",
                           "entities": "a symbol's rank among the store's symbols mod 16",
                           "queries": "members of the store spread evenly over its families, each skipping itself",
                           "warmup_calls": a.warmup, "windows": a.reps, "window_seconds": a.window},
              "timing": "host clock around back-to-back calls on one stream, each window ended by a synchronise; the "
                        "three searches' windows alternate; profiler off. nmz_ed_plan_query_knn takes host arrays "
                        "(it has no device form), so its figure includes its own copies.",
              "shapes": shapes, "host_arrays": host}
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(record, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
