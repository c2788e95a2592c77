"""Wide move-profile rate (a tool, not a bench leg): nmz_move_profile_wide_dev next to nmz_ed_align_wide_pairs_dev
over the stores and pairs of tools/align_wide_rate.py -- clustered traces of 2,048 elements, each with its nearest
neighbour at the band (scripts of a few ops), and the variant whose partner is the trace itself with its first band / 4
elements moved to the end (scripts of about band / 2 ops) -- and the table of every symbol of the store. K9w's rank
and partner loops are quadratic in the script's length, so both ends of it are measured.

Measured, profiler off:
  * (a) bands 65, 128, 512 and 1,024 x 4,096 pairs, both stores: a few warm-up calls, then `--reps` windows of
    back-to-back calls on one stream, each window ended by a synchronise and sized to about `--window` seconds (host
    clock), for the alignment alone and for the profile alone over the alignment's output (d_partner == NULL, as
    nmz_ed_diff_profile_wide calls it), and with an empty table: no lookups that hit and no counter atomics. Reported:
    the median ms per call, its spread, and the profile's time as a share of the alignment's. Before the timing the
    device result is compared with nmz_move_profile_wide_host. Beside the host-clock figures, the kernels alone from
    HIP events around their launches (nmz_timing_enable).
  * (b) host arrays to host counters at 4,096 pairs x 2,048, w = 512, both stores: nmz_ed_diff_profile_wide against
    the only route without it -- edit_scripts_wide, then script_moves and a dict tally per pair in Python --
    alternating, with equal move counts per symbol asserted. The ratio is recorded, not gated.
usage: python3 tools/moves_wide_rate.py [--out profiles/moves_wide/rate.json]
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
from align_wide_rate import LENGTH, nearest_pairs  # noqa: E402
from moves_rate import KERNEL_CALLS, kernel_ms  # noqa: E402
from order_rate import windows  # noqa: E402

BANDS = [65, 128, 512, 1024]
PARENT_BAND = 512


def python_route(ts, pairs, band, ctx):
    """edit_scripts_wide, then script_moves and a dict tally per pair: {symbol: moves}."""
    es = hs.edit_scripts_wide(ts, pairs, band, ctx=ctx)
    tally = {}
    for p, (i, j) in enumerate(pairs.tolist()):
        sc = es.script(p)
        if sc is None or len(sc) == 0:
            continue
        for s, _, _ in hs.script_moves(ts.trace(i), ts.trace(j), sc):
            tally[s] = tally.get(s, 0) + 1
    return tally


def one(a, band, P, far, ctx, torch, stream):
    ts = synth.clustered_traces(P, LENGTH, family=min(1024, P // 4))
    if far:  # every trace against itself with its first band / 4 elements moved to the end: about band / 2 edits
        trs = [ts.trace(i) for i in range(P)]
        ts = hs.TraceSet(trs + [np.concatenate([t[band // 4:], t[:band // 4]]) for t in trs])
        pairs = np.stack([np.arange(P, dtype=np.uint32), np.arange(P, 2 * P, dtype=np.uint32)], 1)
    else:
        pairs = nearest_pairs(ts, band, ctx)
    usym = np.unique(ts.sym[:int(ts.off[-1])])
    U = len(usym)
    plan = hs.AlignWidePlan(band, int(np.diff(ts.off.astype(np.int64)).max()), ctx=ctx)
    d_off = torch.from_numpy(ts.off.view(np.int64)).cuda()
    d_sym = torch.from_numpy(ts.sym.view(np.int64)).cuda()
    d_pairs = torch.from_numpy(pairs.view(np.int32)).cuda()
    d_usym = torch.from_numpy(usym.view(np.int64)).cuda()
    d_dist = torch.zeros(P, dtype=torch.int32, device="cuda")
    d_ops = torch.zeros(P * band * 3, dtype=torch.int32, device="cuda")
    d_partner = torch.zeros(P * band, dtype=torch.int32, device="cuda")
    d_counts = torch.zeros(U * 12, dtype=torch.int32, device="cuda")
    d_info = torch.zeros(8, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    L = _lib.load()

    def align():
        plan.pairs_dev(d_off.data_ptr(), d_sym.data_ptr(), d_pairs.data_ptr(), P, d_dist.data_ptr(), d_ops.data_ptr(),
                       stream.cuda_stream)

    def profile(partner=False, n_usym=U):
        _lib.check(L.nmz_move_profile_wide_dev(ctx.handle, d_off.data_ptr(), d_sym.data_ptr(), d_pairs.data_ptr(), P,
                                               band, d_dist.data_ptr(), d_ops.data_ptr(), d_usym.data_ptr(), n_usym,
                                               d_partner.data_ptr() if partner else None, d_counts.data_ptr(),
                                               d_info.data_ptr(), 0, stream.cuda_stream))

    align()
    profile(partner=True)
    stream.synchronize()
    dist = d_dist.cpu().numpy().view(np.uint32)
    ops = d_ops.cpu().numpy().view(_lib.EDIT_OP_DTYPE).reshape(P, band)
    counts = d_counts.cpu().numpy().view(_lib.MOVE_COUNTS_DTYPE)
    info = d_info.cpu().numpy().view(_lib.MOVE_INFO_DTYPE)[0]
    partner = d_partner.cpu().numpy().view(np.uint32).reshape(P, band)
    want = hs.move_profile_of_wide(ts, pairs, hs.EditScripts(dist, ops, band), usym=usym, want_partner=True, host=True)
    assert counts.tobytes() == want.counts.tobytes() and info == want.info, "the profile is wrong"
    assert np.array_equal(partner, want.partner), "the partners are wrong"
    m_al = windows(align, stream.synchronize, a.warmup, a.reps, a.window)
    m_pr = windows(profile, stream.synchronize, a.warmup, a.reps, a.window)
    m_nt = windows(lambda: profile(n_usym=0), stream.synchronize, a.warmup, a.reps, a.window)
    k_al = kernel_ms(ctx, b"ed_align_wide", align, stream)
    k_pr = kernel_ms(ctx, b"script_moves_wide", profile, stream)
    k_nt = kernel_ms(ctx, b"script_moves_wide", lambda: profile(n_usym=0), stream)
    within = dist <= band
    r = {"length": LENGTH, "band": band, "pairs": P, "rotated_partner": far, "table_symbols": U,
         "info": {f: int(info[f]) for f in info.dtype.names},
         "mean_script_ops": float(dist[within].mean()) if within.any() else 0.0,
         "max_script_ops": int(dist[within].max()) if within.any() else 0,
         "moves": int(counts["later"].sum() + counts["earlier"].sum()),
         "align_wide_dev": m_al, "profile_wide_dev": m_pr, "profile_wide_dev_empty_table": m_nt,
         "profile_share_of_align": m_pr["median_ms"] / m_al["median_ms"],
         "result_checked": "nmz_move_profile_wide_host",
         "kernel_only_ms": {"k_ed_align_wide": k_al, "k_script_moves_wide": k_pr,
                            "k_script_moves_wide_empty_table": k_nt, "profile_share_of_align": k_pr / k_al,
                            "how": f"HIP events around the launch alone, mean of {KERNEL_CALLS} calls"}}
    plan.close()
    del d_off, d_sym, d_pairs, d_dist, d_ops, d_partner, d_counts, d_info, d_usym
    line = (f"L={LENGTH} w={band} P={P}{' rotated' if far else ''} U={U}: align {m_al['median_ms']:.3f} ms, profile "
            f"{m_pr['median_ms']:.3f} ms ({r['profile_share_of_align']:.2%} of it; empty table "
            f"{m_nt['median_ms']:.3f}; kernels alone: align {k_al:.3f}, profile {k_pr:.3f}, empty table {k_nt:.3f}), "
            f"mean script {r['mean_script_ops']:.1f} ops, max {r['max_script_ops']}, {r['moves']} moves")
    if band == PARENT_BAND:
        t_new, t_old = [], []
        hs.move_profile_wide(ts, pairs, band, ctx=ctx, usym=usym)
        for _ in range(a.route_reps):
            t0 = time.perf_counter()
            prof = hs.move_profile_wide(ts, pairs, band, ctx=ctx, usym=usym)
            t1 = time.perf_counter()
            tally = python_route(ts, pairs, band, ctx)
            t2 = time.perf_counter()
            t_new.append((t1 - t0) * 1e3)
            t_old.append((t2 - t1) * 1e3)
            moved = prof.counts["later"].astype(np.int64) + prof.counts["earlier"]
            assert {int(s): int(c) for s, c in zip(prof.symbols, moved) if c} == tally, "the two routes disagree"
            assert prof.counts.tobytes() == counts.tobytes()
        r["host_arrays"] = {"ed_diff_profile_wide_ms": t_new, "python_route_ms": t_old,
                            "ed_diff_profile_wide_median_ms": float(np.median(t_new)),
                            "python_route_median_ms": float(np.median(t_old)),
                            "python_over_ed_diff_profile_wide": float(np.median(t_old) / np.median(t_new)),
                            "python_route": "edit_scripts_wide + script_moves + a dict tally per pair",
                            "moves_per_symbol_equal": True}
        line += (f"  host arrays: ed_diff_profile_wide {np.median(t_new):.2f} ms, python route "
                 f"{np.median(t_old):.1f} ms ({r['host_arrays']['python_over_ed_diff_profile_wide']:.1f}x)")
    print(line, flush=True)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=4096)
    ap.add_argument("--bands", type=int, nargs="+", default=BANDS)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--route-reps", type=int, default=3)
    ap.add_argument("--window", type=float, default=0.25)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "moves_wide", "rate.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("moves_wide_rate.py measures on the GPU; no device found")
    ctx = _lib.Context(0)
    stream = torch.cuda.Stream()
    shapes = {}
    for band in a.bands:
        for far in (False, True):
            shapes[f"L{LENGTH}_w{band}_P{a.pairs}{'_rotated' if far else ''}"] = one(a, band, a.pairs, far, ctx, torch,
                                                                                  stream)
    record = {"workload": {"generator": "namazu_amd/synth.clustered_traces (the bench's configs[2] clustered leg)",
                           "pairs": "each trace with its nearest neighbour at the band (nmz_ed_allpairs_knn, k = 1); "
                                    "rotated: each trace with itself, its first band / 4 elements moved to the end",
                           "table": "every symbol of the store", "warmup_calls": a.warmup, "windows": a.reps,
                           "window_seconds": a.window},
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
