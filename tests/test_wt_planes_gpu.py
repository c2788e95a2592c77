"""GPU parity of K1's rank-block planes (replayable_wt.hip: 64-rank blocks, planes in place of the levels while the row
image stays within 128 KB): every case sweeps 4,096 seeds through nmz_replayable_sweep_topk_dev and asserts stats and
top-k bit for bit against the oracle, for the plane form and for the level form of the same plan (NMZ_WT_PLANES=0),
built by the fused plan kernel and by the separate one (NMZ_WT_FUSED=0); nmz_replayable_plan_wt_info says which form
ran. One-length-class traces sit where the planes change shape: a single block (planes 0 and NB only), one real plane,
a last block of one rank or none, more than one 32-position word per plane, 47 blocks (six search steps). A single
class of 4,095 events needs a 140 KB image (64.5 KB of planes, 33 KB of masks, 41 KB of Cm, C_hi and e) and so keeps
its levels, like two such classes. maxInterval 3 forces ties and wholly wrapping parts, 2^31 + 5 the BIG kernel form."""
import ctypes

import numpy as np
import pytest

from namazu_amd import _lib
from namazu_amd.explorepolicy import to_csr
from oracle import oracle as O

pytestmark = pytest.mark.gpu

PLANES_MAX = 128 * 1024  # csrc/replayable_wt_dev.h: WT_PLANES_MAX
MS = (3, 1000, 100_000_000, 2**31 + 5)
SEEDS = [str(i * 7919 + 1) for i in range(4096)]


def class_hints(sizes, seed):
    """hints in len(sizes) length classes (19 + c digits), sizes[c] distinct hints each, in a shuffled order"""
    rng = np.random.default_rng(seed)
    out = []
    for c, n in enumerate(sizes):
        w = 19 + c
        v = rng.choice(10**9, size=n, replace=False)
        out += [("%09d" % x).rjust(w, "7") for x in v]
    return [out[i] for i in rng.permutation(len(out))]


def run_plan(ctx, hints, m, seeds, k):
    """one plan, one sweep: (bb, planes, image bytes), stats, top-k"""
    import torch
    L = _lib.load()
    ho, hb = to_csr(hints)
    so, sb = to_csr(seeds)
    S = len(seeds)
    plan = ctypes.c_void_p()
    _lib.check(L.nmz_replayable_plan_create(ctx.handle, _lib.ptr(ho), _lib.ptr(hb), len(hints), m, S,
                                            ctypes.byref(plan)))
    try:
        assert L.nmz_replayable_plan_kernel(plan) == 2
        bb, planes, nbytes = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint64()
        _lib.check(L.nmz_replayable_plan_wt_info(plan, ctypes.byref(bb), ctypes.byref(planes), ctypes.byref(nbytes)))
        d_so = torch.from_numpy(so.view(np.int32)).cuda()
        d_sb = torch.from_numpy(sb).cuda()
        d_st = torch.zeros(S * 32, dtype=torch.uint8, device="cuda")
        d_tk = torch.zeros(k * 24, dtype=torch.uint8, device="cuda")
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        _lib.check(L.nmz_replayable_sweep_topk_dev(plan, ctypes.c_void_p(d_so.data_ptr()),
                                                   ctypes.c_void_p(d_sb.data_ptr()), S, 0, k,
                                                   ctypes.c_void_p(d_st.data_ptr()), ctypes.c_void_p(d_tk.data_ptr()),
                                                   stream))
        torch.cuda.synchronize()
        st = np.frombuffer(d_st.cpu().numpy().tobytes(), dtype=_lib.SCHED_STATS_DTYPE)
        tk = np.frombuffer(d_tk.cpu().numpy().tobytes(), dtype=_lib.TOPK_DTYPE)
    finally:
        L.nmz_replayable_plan_destroy(plan)
    return (bb.value, planes.value, nbytes.value), st, tk


def check_forms(ctx, monkeypatch, hints, m, seeds, want_planes, k=16):
    """the plan in its default form and with NMZ_WT_PLANES=0, from both plan builders, against the oracle"""
    so, sb = O.to_csr(seeds)
    ho, hb = O.to_csr(hints)
    ost = O.replayable_sweep(so, sb, ho, hb, m, n_dump=0)[0]
    exp = O.topk_from_stats(ost, 0, k)
    for planes_env in (None, "0"):
        for fused_env in (None, "0"):
            for name, val in (("NMZ_WT_PLANES", planes_env), ("NMZ_WT_FUSED", fused_env)):
                if val is None:
                    monkeypatch.delenv(name, raising=False)
                else:
                    monkeypatch.setenv(name, val)
            (bb, planes, nbytes), st, tk = run_plan(ctx, hints, m, seeds, k)
            what = (len(hints), m, planes_env, fused_env)
            assert planes == (1 if want_planes and planes_env is None else 0), what
            assert not planes or (bb == 6 and nbytes <= PLANES_MAX), what
            assert st.tobytes() == ost.tobytes(), what
            assert tk.tolist() == exp.tolist(), what


@pytest.mark.parametrize("n", [9, 63, 64, 65, 127, 128, 129, 200, 1030, 3000, 4095])
@pytest.mark.parametrize("m", MS)
def test_one_length_class(ab_knobs, ctx, monkeypatch, n, m):
    check_forms(ctx, monkeypatch, class_hints([n], n), m, SEEDS, want_planes=n != 4095)


def test_two_classes_over_the_image_budget(ab_knobs, ctx, monkeypatch):
    """Two 4,095-event classes: 129 KB of planes alone, so the plan keeps its levels (and, their image past LDS with
    64-rank blocks, takes 32-rank blocks), and the output is still exact."""
    check_forms(ctx, monkeypatch, class_hints([4095, 4095], 5), 100_000_000, SEEDS, want_planes=False)


@pytest.mark.parametrize("m", (100_000_000, 2**31 + 5))
def test_configs1_shaped_mix(ab_knobs, ctx, monkeypatch, m):
    """Five classes of the flagship trace's sizes: two large plane segments, a small one, and two that are too short
    for an image (25 events: levels or planes of one block; 4: per-event decisions)."""
    seeds = [str(i * 104_729 + 3) for i in range(8192)]
    check_forms(ctx, monkeypatch, class_hints([2079, 1785, 203, 25, 4], 6), m, seeds, want_planes=True, k=64)
