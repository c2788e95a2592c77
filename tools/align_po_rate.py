"""Per-entity (partial-order) edit-script rate (a tool, not a bench leg): nmz_po_project_dev and
nmz_ed_align_po_pairs_dev over clustered stores of 2,048 events with 16 entities (the generator of the bench's
configs[2] clustered leg, namazu_amd/synth.clustered_traces; a symbol's entity is its rank among the store's symbols
mod 16, so a symbol determines its entity as an event does) -- tools/align_wide_rate.py's pattern.

Measured, profiler off:
  * the projection alone (count pass, scan, scatter pass) over the whole store: ms per call and GB/s beside the
    bytes-moved bound of DESIGN.md section 4, K10 -- 12 B in per element on each pass and 12 B out on the scatter;
  * PO scripts at bands 32, 128 and 512 per 4,096 pairs (each trace with its nearest neighbour at the band), beside
    nmz_ed_align_wide_pairs_dev over the same pairs in the same run, alternating window for window;
  * host arrays to host arrays: nmz_ed_align_po_pairs against the only earlier route -- project in numpy, run
    edit_scripts_wide on the projected TraceSet, lift and concatenate in numpy. Results must be equal (asserted).
Ratios are recorded, not gated.
usage: python3 tools/align_po_rate.py [--out profiles/align_po/rate.json]
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
from align_wide_rate import nearest_pairs  # noqa: E402
from order_rate import windows  # noqa: E402

LENGTH = 2048
ENTITIES = 16
BANDS = [32, 128, 512]
BOUND_BYTES_PER_ELEMENT = 12 + 12 + 12  # count pass in, scatter pass in, scatter pass out


def numpy_project(ts, ent, G):
    """(projected TraceSet-like off / sym, psrc) by a stable sort on (trace, entity)."""
    T, N = len(ts), int(ts.off[-1])
    lens = np.diff(ts.off.astype(np.int64))
    trace = np.repeat(np.arange(T), lens)
    keep = np.nonzero(ent[:N] != _lib.NMZ_NONE)[0]
    key = trace[keep] * G + ent[keep].astype(np.int64)
    order = keep[np.argsort(key, kind="stable")]
    poff = np.zeros(T * G + 1, np.uint64)
    poff[1:] = np.cumsum(np.bincount(key, minlength=T * G))
    return poff, ts.sym[order], (order - ts.off.astype(np.int64)[trace[order]]).astype(np.uint32)


def numpy_route(ts, ent, G, pairs, band, ctx):
    """The earlier route, host arrays to host arrays: numpy projection, edit_scripts_wide over the sub-pairs, numpy
    lift and concatenation."""
    P = len(pairs)
    poff, psym, psrc = numpy_project(ts, ent, G)
    proj = hs.TraceSet([])
    proj.off, proj.sym = poff, (psym if len(psym) else np.zeros(1, np.uint64))
    g = np.arange(G, dtype=np.uint32)
    sub = np.stack([(pairs[:, 0:1] * G + g).reshape(-1), (pairs[:, 1:2] * G + g).reshape(-1)], 1).astype(np.uint32)
    es = hs.edit_scripts_wide(proj, sub, band, ctx=ctx)
    sd = es.dist.reshape(P, G).astype(np.int64)
    total = np.minimum(sd, band + 1).sum(axis=1)
    dist = np.where(total > band, band + 1, total).astype(np.uint32)
    ops = np.zeros((P, band), _lib.EDIT_OP_DTYPE)
    ops[:] = (_lib.NMZ_NONE,) * 3
    so = es.ops.reshape(P, G, band)
    live = (np.arange(band)[None, None, :] < sd[:, :, None]) & (total <= band)[:, None, None]
    pi, gi, si = np.nonzero(live)
    src = so[pi, gi, si]
    lens = np.diff(ts.off.astype(np.int64))
    for side, col in ((0, "a_pos"), (1, "b_pos")):
        q = pairs[pi, side].astype(np.int64) * G + gi
        lo, n_g = poff[q].astype(np.int64), (poff[q + 1] - poff[q]).astype(np.int64)
        pos = src[col].astype(np.int64)
        inside = pos < n_g
        src[col] = np.where(inside, psrc[np.where(inside, lo + pos, 0)], lens[pairs[pi, side]]).astype(np.uint32)
    start = np.concatenate([[0], np.cumsum(live.reshape(P, -1).sum(axis=1))])[:-1]
    ops[pi, np.arange(len(pi)) - start[pi]] = src
    return dist, ops


def fold(ms):
    v = [x["median_ms"] for x in ms]
    med = float(np.median(v))
    return {"ms_per_call": v, "median_ms": med, "spread": (max(v) - min(v)) / med,
            "calls_per_window": [x["sweeps_per_window"] for x in ms]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=4096)
    ap.add_argument("--bands", type=int, nargs="+", default=BANDS)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-reps", type=int, default=2)
    ap.add_argument("--window", type=float, default=0.25)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "align_po", "rate.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("align_po_rate.py measures on the GPU; no device found")
    ctx = _lib.Context(0)
    stream = torch.cuda.Stream()
    P, G = a.pairs, ENTITIES
    ts = synth.clustered_traces(P, LENGTH, family=min(1024, P // 4))
    N = int(ts.off[-1])
    ent = (np.searchsorted(np.unique(ts.sym[:N]), ts.sym[:N]) % G).astype(np.uint32)
    max_len = int(np.diff(ts.off.astype(np.int64)).max())
    d_off = torch.from_numpy(ts.off.view(np.int64)).cuda()
    d_sym = torch.from_numpy(ts.sym.view(np.int64)).cuda()
    d_ent = torch.from_numpy(ent.view(np.int32)).cuda()
    d_poff = torch.zeros(P * G + 1, dtype=torch.int64, device="cuda")
    d_psym = torch.zeros(N + 1, dtype=torch.int64, device="cuda")
    d_psrc = torch.zeros(N + 1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    L = _lib.load()

    def project():
        import ctypes
        _lib.check(L.nmz_po_project_dev(ctx.handle, ctypes.c_void_p(d_off.data_ptr()), ctypes.c_void_p(d_sym.data_ptr()),
                                        ctypes.c_void_p(d_ent.data_ptr()), P, G, ctypes.c_void_p(d_poff.data_ptr()),
                                        ctypes.c_void_p(d_psym.data_ptr()), ctypes.c_void_p(d_psrc.data_ptr()),
                                        ctypes.c_void_p(stream.cuda_stream)))

    project()
    stream.synchronize()
    want = numpy_project(ts, ent, G)
    assert np.array_equal(d_poff.cpu().numpy().view(np.uint64), want[0])
    assert np.array_equal(d_psym.cpu().numpy().view(np.uint64)[:N], want[1])
    assert np.array_equal(d_psrc.cpu().numpy().view(np.uint32)[:N], want[2])
    m = fold([windows(project, stream.synchronize, a.warmup if r == 0 else 1, 1, a.window) for r in range(a.reps)])
    bound = N * BOUND_BYTES_PER_ELEMENT
    projection = dict(m, traces=P, length=LENGTH, entities=G, elements=N, bound_bytes=bound,
                      bound_gb_per_s=bound / m["median_ms"] / 1e6, results_equal_numpy=True)
    print(f"projection: {P} x {LENGTH}, {G} entities: {m['median_ms']:.3f} ms/call (spread {m['spread']:.2%}), "
          f"{projection['bound_gb_per_s']:.0f} GB/s of the {bound / 1e6:.0f} MB bound", flush=True)
    shapes = {}
    for band in a.bands:
        pairs = nearest_pairs(ts, band, ctx)
        plan, wide = hs.AlignPoPlan(band, G, max_len, P, ctx=ctx), hs.AlignWidePlan(band, max_len, ctx=ctx)
        d_pairs = torch.from_numpy(pairs.view(np.int32)).cuda()
        d_dist = torch.zeros(P, dtype=torch.int32, device="cuda")
        d_ops = torch.zeros(P * band * 3, dtype=torch.int32, device="cuda")
        w_dist = torch.zeros(P, dtype=torch.int32, device="cuda")
        w_ops = torch.zeros(P * band * 3, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()

        def step():
            plan.pairs_dev(d_off.data_ptr(), d_poff.data_ptr(), d_psym.data_ptr(), d_psrc.data_ptr(), d_pairs.data_ptr(),
                           P, d_dist.data_ptr(), d_ops.data_ptr(), stream.cuda_stream)

        def step_wide():
            wide.pairs_dev(d_off.data_ptr(), d_sym.data_ptr(), d_pairs.data_ptr(), P, w_dist.data_ptr(), w_ops.data_ptr(),
                           stream.cuda_stream)

        step()
        step_wide()
        stream.synchronize()
        dist = d_dist.cpu().numpy().view(np.uint32)
        ops = d_ops.cpu().numpy().view(_lib.EDIT_OP_DTYPE).reshape(P, band)
        wd = w_dist.cpu().numpy().view(np.uint32)
        m_p, m_w = [], []
        for r in range(a.reps):  # alternating, one window each per round, so that both see the same machine
            m_p.append(windows(step, stream.synchronize, a.warmup if r == 0 else 1, 1, a.window))
            m_w.append(windows(step_wide, stream.synchronize, a.warmup if r == 0 else 1, 1, a.window))
        mp, mw = fold(m_p), fold(m_w)
        r = {"length": LENGTH, "band": band, "pairs": P, "entities": G, "slots": plan.slots,
             "history_bytes": plan.history_bytes, "sub_pair_bytes": plan.sub_pair_bytes,
             "in_band_fraction": float((dist <= band).mean()),
             "mean_script_ops": float(dist[dist <= band].mean()) if (dist <= band).any() else 0.0,
             "exact_mean_script_ops": float(wd[wd <= band].mean()) if (wd <= band).any() else 0.0,
             "align_po_dev": mp, "pairs_per_s": P / mp["median_ms"] * 1e3,
             "align_wide_dev": dict(mw, slots=wide.slots, pairs_per_s=P / mw["median_ms"] * 1e3),
             "po_over_wide": mp["median_ms"] / mw["median_ms"]}
        plan.close()
        wide.close()
        del d_pairs, d_dist, d_ops, w_dist, w_ops
        t_po, t_np = [], []
        for _ in range(a.host_reps):
            t0 = time.perf_counter()
            es = hs.edit_scripts_po(ts, ent, pairs, band, n_entities=G, ctx=ctx)
            t1 = time.perf_counter()
            nd, no = numpy_route(ts, ent, G, pairs, band, ctx)
            t2 = time.perf_counter()
            t_po.append((t1 - t0) * 1e3)
            t_np.append((t2 - t1) * 1e3)
            assert np.array_equal(es.dist, dist) and es.ops.tobytes() == ops.tobytes(), \
                "the host-pointer and the device-pointer form disagree"
            assert np.array_equal(nd, dist) and no.tobytes() == ops.tobytes(), "the numpy route and the device disagree"
        r["host_arrays"] = {"ed_align_po_pairs_ms": t_po, "numpy_route_ms": t_np,
                            "ed_align_po_pairs_median_ms": float(np.median(t_po)),
                            "numpy_route_median_ms": float(np.median(t_np)),
                            "numpy_route_over_po_pairs": float(np.median(t_np) / np.median(t_po)),
                            "results_equal": True}
        shapes[f"L{LENGTH}_w{band}_P{P}_G{G}"] = r
        print(f"L={LENGTH} w={band} P={P} G={G}: po dev {mp['median_ms']:.3f} ms/call (spread {mp['spread']:.2%}, "
              f"{r['pairs_per_s']:.4g} pairs/s)  wide dev {mw['median_ms']:.3f} ms/call  host arrays: "
              f"ed_align_po_pairs {np.median(t_po):.1f} ms, numpy route {np.median(t_np):.1f} ms", flush=True)
    record = {"workload": {"generator": "namazu_amd/synth.clustered_traces (the bench's configs[2] clustered leg)",
                           "entities": "a symbol's rank among the store's symbols mod 16",
                           "pairs": "each trace with its nearest neighbour at the band (nmz_ed_allpairs_knn, k = 1)",
                           "warmup_calls": a.warmup, "windows": a.reps, "window_seconds": a.window},
              "timing": "host clock around back-to-back calls on one stream, each window ended by a synchronise; the "
                        "PO plan's windows alternate with the wide plan's; profiler off",
              "projection": projection, "shapes": shapes}
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(record, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
