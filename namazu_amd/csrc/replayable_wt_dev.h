// K1 wavelet-tree statistics: what the plan kernel (replayable_wt_plan.hip), the sweep (replayable_wt.hip) and the
// selection (replayable_wt_topk_dev.h) share -- the row image's sizes and limits, and the top-k scratch the sweep writes
// and the selection reads. replayable_plan.h holds what replayable.hip sees (WtState, WtClass, the entry points).
#pragma once
#include "nmz_common.h"
#include "nmz_internal.h"
#include "replayable_plan.h"

namespace nmz {

#ifndef NMZ_WT_BRUTE
#define NMZ_WT_BRUTE 8
#endif
// segments of at most this many events: per-event decisions (32, for configs[1]'s 25-event segment: K1 0.062 ->
// 0.0675 ms, profiles/r05/k1/brute_ab)
constexpr uint32_t WT_BRUTE = NMZ_WT_BRUTE;
constexpr uint32_t WT_NMAX = 4096;     // largest segment the plan kernel sorts in LDS
constexpr uint32_t WT_LDS_MAX = 160 * 1024 - 256;  // dynamic LDS; the sweep kernel's few static bytes need the rest
constexpr uint32_t WT_NONE = 0xffffffffu;
constexpr uint32_t WT_PAD = 32;  // sentinels past Cm and C_hi: lifting searches of <= 5 rounds need no clamp

// The tree stores the levels above the rank blocks of 2^bb ranks (bb = 5, 6 or 7: 32-, 64- or 128-rank blocks, the
// plan's choice, wt_layout); the blocks' prefix masks stand for the last bb levels. A wider block takes levels off
// both descents (each level one dependent LDS read per chain) for a larger image: ~2^bb / 8 bytes of masks per
// event (4, 8, 16). configs[1] (profiles/r05/k1/blocks_ab): bb = 6 takes K1 0.0656 -> 0.0623 ms and the pipelined
// step 0.0721 -> 0.0712 ms (84 KB images); bb = 7 (118 KB) runs K1 at 0.066 ms (its 128-bit mask arithmetic) and
// leaves the step's other kernels too little LDS beside it (step 0.082 ms), so plans take at most bb = 6.
__host__ __device__ constexpr uint32_t wt_levels(uint32_t K, uint32_t bb) { return K > bb ? K - bb : 0; }
// block masks' bytes: (n >> bb) + 1 blocks of 2^bb + 1 prefix masks of 2^bb bits
__host__ __device__ constexpr uint64_t wt_mask_bytes(uint32_t n, uint32_t bb) {
    return (uint64_t)((n >> bb) + 1) * ((1u << bb) + 1) * ((1u << bb) / 8);
}

// Rank-block planes (64-rank blocks only) replace the levels of a plan whose row image stays small enough: with
// NB = (n >> 6) + 1 blocks, plane b (b = 0 .. NB) holds bit i = [rank_i >= 64 b] in position order, stored like a
// level, so f_b(d) = #{i < d: rank_i >= 64 b} is one read and a count needs two dependent rounds (two planes, one
// mask) instead of a descent of K - 6 levels. Plane bytes grow as n^2 / 256 (16.6 KB for 2,079 events against 3.1 KB
// of levels; 65 KB for 4,095).
__host__ __device__ constexpr uint64_t wt_plane_bytes(uint32_t n, uint32_t nw) {
    return (uint64_t)((n >> 6) + 2) * nw * 8;
}
// One K1 workgroup's row image and the 26.7 KB of static LDS of k_wt_topk_chunks must fit a CU's 160 KB together, or
// the selection of the neighbouring step waits for a whole CU (the 118 KB images of 128-rank blocks cost the
// pipelined step that overlap): planes are taken only while the row image is at most 128 KB.
constexpr uint64_t WT_PLANES_MAX = 128 * 1024;

// Images above 64 KB need the dynamic-LDS attribute on every kernel form that stages or builds one. wt_layout sets it
// once per context: on the plan kernel's forms itself, on the sweep's through this (replayable_wt.hip; false: a form
// refused it, and the error is still pending).
bool wt_sweep_lds_attr();

// ---- the top-k scratch (wt_topk_scratch_bytes(S)): the selection's candidate arrays, then one record per chunk of
// 64 WT_NS seeds, written by the sweep at slot chunk_base[L] + ch and read by the selection ----
constexpr uint32_t WT_CAND = 4096;
constexpr int WT_NS = 1;  // seeds per lane of the sweep: its chunks hold 64 WT_NS seeds
struct WtChunkRec {
    unsigned long long key;  // the chunk's largest sum ^ 2^63
    uint32_t pos, cnt;       // sorted position of the chunk's first seed; its seeds
};
static_assert(sizeof(WtChunkRec) == 16, "WtChunkRec layout");
struct WtTopkState {
    unsigned long long cand_key[WT_CAND];
    uint32_t cand_idx[WT_CAND];
};
// every row's last chunk may be partial
inline uint64_t wt_max_chunks(uint64_t S) { return S / (64 * WT_NS) + 256; }

struct WtTopkScratch {
    WtTopkState *tk;
    WtChunkRec *rec;  // [wt_max_chunks(S)]
    size_t bytes;     // of the whole scratch
};
// the one carve of the scratch (p == nullptr: only the size is wanted)
inline WtTopkScratch wt_topk_carve(void *p, uint64_t S) {
    WtTopkScratch s{};
    ScratchLayout lay;
    lay.add(&s.tk, 1).add(&s.rec, wt_max_chunks(S));
    s.bytes = lay.bytes();
    if (p) (void)lay.place(p);
    return s;
}

}  // namespace nmz
