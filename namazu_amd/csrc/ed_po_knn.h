// What the two PO k-NN search kernels share: K11b (k_po_knn, ed_po_knn.hip; one wave per pair, bands 0 .. 64) and
// K11w (k_po_knn_wide, ed_po_knn_wide.hip; four waves per pair, bands 65 .. 1,024). One argument block, one filter,
// one set of counters; the plan, its validators, the batcher and the enqueue are ed_po_knn.hip's and serve both.
#pragma once
#include "ed_plan.h"
#include "nmz_common.h"

namespace nmz {

constexpr uint32_t PK_ITEMS_PER_WAVE = 4;  // the deal's aim: at least this many items per persistent wave / workgroup
constexpr uint32_t PK_PROF_WORDS = 64;     // 32 lenfold words + 128 gram bytes
constexpr uint32_t PK_NCOUNTERS = 4;
// K11w's counters behind K11's four: the entity steps at C = 1, 2, 3, 5, 9 cells per thread
constexpr uint32_t PKW_NCOUNTERS = NMZ_PO_KNN_WIDE_NCOUNTERS, PKW_NSTEPS = PKW_NCOUNTERS - PK_NCOUNTERS;
static_assert(PKW_NCOUNTERS <= ED_CNT_LINE, "a stripe of the counters is one line");

struct PkArgs {
    const uint64_t *poff, *psym;  // the store, projected
    const uint32_t *prof;
    const uint64_t *q_poff, *q_psym;  // the queries, projected
    const uint32_t *q_prof;
    const uint32_t *q_self;  // may be NULL
    uint32_t N, G, k, w, no_filter, NB, parts;
    uint64_t n_items;  // n_queries * NB * parts
    uint64_t *knn;
    uint64_t *counters;                // [ED_CNT_WORDS]
    unsigned long long *next;          // the item counter
    const uint32_t *over;              // the guard's flag
    uint32_t full_band;                // K11w: every entity laid out for w (NMZ_PO_KNN_OPT_FULL_BAND)
};

__device__ __forceinline__ uint32_t pk_wave_sum(uint32_t v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ uint64_t pk_lane64(uint64_t v, int src) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, src);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), src);
    return ((uint64_t)hi << 32) | lo;
}

// The filter, a lane per candidate: the query's profile qp is uniform, the lane reads its candidate's 256 bytes cp.
// max(LB_len, LB_gram) <= w: the pair goes on to the DP.
__device__ __forceinline__ bool pk_filter_passes(const uint32_t *__restrict__ qp, const uint4 *__restrict__ cp,
                                                 uint32_t w) {
    uint64_t lb_len = 0;
    uint32_t sad = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const uint4 c = cp[i];
        const uint32_t a0 = qp[4 * i], a1 = qp[4 * i + 1], a2 = qp[4 * i + 2], a3 = qp[4 * i + 3];
        lb_len += (c.x > a0 ? c.x - a0 : a0 - c.x);
        lb_len += (c.y > a1 ? c.y - a1 : a1 - c.y);
        lb_len += (c.z > a2 ? c.z - a2 : a2 - c.z);
        lb_len += (c.w > a3 ? c.w - a3 : a3 - c.w);
    }
#pragma unroll
    for (int i = 8; i < 16; ++i) {
        const uint4 c = cp[i];
        sad = __builtin_amdgcn_sad_u8(c.x, qp[4 * i], sad);
        sad = __builtin_amdgcn_sad_u8(c.y, qp[4 * i + 1], sad);
        sad = __builtin_amdgcn_sad_u8(c.z, qp[4 * i + 2], sad);
        sad = __builtin_amdgcn_sad_u8(c.w, qp[4 * i + 3], sad);
    }
    const uint64_t lb_gram = (sad + 3) / 4;
    return (lb_len > lb_gram ? lb_len : lb_gram) <= w;
}

// ---- K11w's launch (ed_po_knn_wide.hip), for pk_enqueue; the caller holds the context ----
// the workgroups of k_po_knn_wide that the device keeps resident for a plan of this band
uint64_t pkw_resident(const nmz_ctx *ctx, uint32_t band);
// 64 < a.w <= 1,024; blocks <= pkw_resident(ctx, a.w)
int pkw_launch(nmz_ctx *ctx, hipStream_t st, const PkArgs &a, unsigned blocks);

}  // namespace nmz
