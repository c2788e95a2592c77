// K9w -- move profiles over scripts wider than one wave holds: 64 < band <= 1,024
// (historystorage/historystorage.go:50-51 is the search interface this extends, naive/naive.go:235-257 the
// reference's equality search, naive.go:199-213 the labels that make "failing against its nearest passing run").
//
// The semantics are K9's (ed_moves.hip; DESIGN.md section 2, "Move profiles") word for word, over K8w's output:
// dist[P] and ops[P][band] (ed_align_wide.hip). The nmz_move_profile_wide_* entry points take every band 0 .. 1,024;
// a band <= 64 runs k_script_moves, so it gives the narrow entry points' bytes.
//
// k_script_moves_wide<LDS>: K9 one level up. One workgroup of 256 threads (4 waves) per
// pair, grid-striding over the pairs. Thread tid owns slots tid + 256 c, c < 4. Per script (1 <= dist <= band):
//   1. stage: the thread loads its ops, turns a kind > 2 or a position outside its trace into a sentinel before
//      anything is read through it, loads the one or two symbols each op names and writes kind, va, vb and b_pos of
//      its slots to LDS (28 KiB for 1,024 slots, the ranks included);
//   2. rank: one loop over the slots t < dist. t is workgroup-uniform, so the LDS reads are same-address broadcasts;
//      per owned slot the thread counts the equal (kind, value) ops in lower slots -- its rank -- and learns whether
//      a lower slot names either of its values (the first slot naming a value counts n_pairs). Only lower slots
//      count, so a wave stops at its own highest owned slot;
//   3. partner: only if the script holds both DELs and INSs (two workgroup votes). The ranks go to LDS and a second
//      loop of the same kind finds the slot with (opposite kind, value, rank); the span reads its b_pos from LDS;
//   4. tally: K9's. The names are looked up in usym by binary search -- in LDS when the table has at most
//      MV_LDS_SYMS entries, staged once per workgroup -- and the counters take integer atomicAdds (sums: the result
//      is deterministic). partner goes out with plain stores, all `band` slots of the pair; info is summed per
//      workgroup in LDS and takes at most four global atomics per workgroup at the end. No scratch, nothing
//      allocated per launch.
// Both loops are quadratic in the script's length (not in the band): K9's algorithm, whose cost beside the
// alignment is measured in DESIGN.md section 4.
#include <algorithm>
#include <string>

#include "ed_plan.h"
#include "nmz_common.h"
#include "nmz_internal.h"

namespace nmz {

constexpr uint32_t MW_THREADS = 256;  // 4 waves
constexpr uint32_t MW_C = NMZ_ALIGN_WIDE_MAX_BAND / MW_THREADS;  // slots per thread
constexpr uint32_t MW_SLOTS = MW_THREADS * MW_C;
// workgroups a CU holds at once: 160 KiB of LDS over 44.1 KiB (table staged) or 28.1 KiB (table in global memory)
constexpr uint32_t MW_BLOCKS_PER_CU_LDS = 3, MW_BLOCKS_PER_CU_GLOBAL = 5;
static_assert(NMZ_ALIGN_WIDE_MAX_BAND == 1024 && MW_SLOTS == NMZ_ALIGN_WIDE_MAX_BAND,
              "a pair's ops fit one workgroup: four slots per thread");

template <bool LDS>
__global__ __launch_bounds__(MW_THREADS) void k_script_moves_wide(const MvArgs g) {
    __shared__ uint64_t s_tab[LDS ? MV_LDS_SYMS : 1];
    __shared__ uint64_t s_va[MW_SLOTS], s_vb[MW_SLOTS];
    __shared__ uint32_t s_kind[MW_SLOTS], s_bp[MW_SLOTS], s_rank[MW_SLOTS];
    __shared__ unsigned long long s_info[4];  // the workgroup's n_scripts, n_beyond, n_ops, n_unknown
    const uint32_t tid = threadIdx.x;
    if (tid < 4) s_info[tid] = 0;
    if (LDS)
        for (uint64_t i = tid; i < g.n_usym; i += MW_THREADS) s_tab[i] = g.usym[i];
    __syncthreads();
    const uint32_t wv = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid >> 6));
    const uint32_t band = g.band;
    uint64_t n_scripts = 0, n_beyond = 0, n_ops = 0;  // workgroup-uniform, over the workgroup's pairs
    uint32_t n_unknown = 0;                           // this thread's

    for (uint64_t p = blockIdx.x; p < g.n_pairs; p += gridDim.x) {
        const uint32_t d = (uint32_t)__builtin_amdgcn_readfirstlane((int)g.dist[p]);
        uint32_t pr[MW_C];
#pragma unroll
        for (uint32_t c = 0; c < MW_C; ++c) pr[c] = NMZ_NONE;
        if (d > band) {
            ++n_beyond;
        } else {
            ++n_scripts;
            n_ops += d;
        }
        if (d >= 1 && d <= band && d <= MW_SLOTS) {
            const uint32_t ia = g.pairs[2 * p], ib = g.pairs[2 * p + 1];
            const uint64_t alo = g.off[ia], ahi = g.off[ia + 1], blo = g.off[ib], bhi = g.off[ib + 1];
            const uint64_t n = ahi > alo ? ahi - alo : 0, m = bhi > blo ? bhi - blo : 0;
            // ---- stage: this thread's slots, sanitised, then their names
            uint32_t kind[MW_C], bp[MW_C];
            uint64_t va[MW_C], vb[MW_C];
            __syncthreads();  // the pair before is done with the staged script
#pragma unroll
            for (uint32_t c = 0; c < MW_C; ++c) {
                const uint32_t s = tid + MW_THREADS * c;
                uint32_t ap = 0, bq = 0, k = NMZ_NONE;
                if (s < d) {
                    const nmz_edit_op *__restrict__ o = g.ops + p * band + s;
                    ap = o->a_pos;
                    bq = o->b_pos;
                    k = o->kind;
                }
                // a kind > 2 or a position outside its trace: the op counts for nothing. One select decides the
                // kind that every later step sees; the names are read only behind it.
                const bool needA = k == NMZ_EDIT_SUB || k == NMZ_EDIT_DEL;
                const bool needB = k == NMZ_EDIT_SUB || k == NMZ_EDIT_INS;
                const bool ok = (needA || needB) && (!needA || ap < n) && (!needB || bq < m);
                kind[c] = ok ? k : NMZ_NONE;
                bp[c] = bq;
                va[c] = ok && needA ? g.sym[alo + ap] : 0;
                vb[c] = ok && needB ? g.sym[blo + bq] : 0;
                if (s < d) {
                    s_kind[s] = kind[c];
                    s_va[s] = va[c];
                    s_vb[s] = vb[c];
                    s_bp[s] = bp[c];
                }
            }
            __syncthreads();
            // ---- rank among equal (kind, value) ops in lower slots; does a lower slot name va / vb?
            uint32_t rank[MW_C];
            bool seenA[MW_C], seenB[MW_C];
#pragma unroll
            for (uint32_t c = 0; c < MW_C; ++c) rank[c] = 0, seenA[c] = seenB[c] = false;
            // the wave's highest live slot: lane 63 of the last c whose first lane is below d
            const uint32_t w0 = wv * 64;
            const uint32_t cl = d > w0 ? (d - 1 - w0) / MW_THREADS : 0;
            const uint32_t t_end = d > w0 ? min(d - 1, w0 + MW_THREADS * cl + 63) : 0;
            for (uint32_t t = 0; t < t_end; ++t) {
                const uint32_t kt = s_kind[t];
                if (kt == NMZ_NONE) continue;
                const uint64_t at = s_va[t], bt = s_vb[t];
#pragma unroll
                for (uint32_t c = 0; c < MW_C; ++c) {
                    const bool below = t < tid + MW_THREADS * c;
                    const bool hasA = kind[c] == NMZ_EDIT_SUB || kind[c] == NMZ_EDIT_DEL;
                    const bool hasB = kind[c] == NMZ_EDIT_SUB || kind[c] == NMZ_EDIT_INS;
                    if (kt != NMZ_EDIT_INS) {  // slot t names a[a_pos]
                        const bool eA = hasA && at == va[c], eB = hasB && at == vb[c];
                        seenA[c] = seenA[c] || (below && eA);
                        seenB[c] = seenB[c] || (below && eB);
                        if (kt == NMZ_EDIT_DEL && kind[c] == NMZ_EDIT_DEL && below && eA) ++rank[c];
                    }
                    if (kt != NMZ_EDIT_DEL) {  // slot t names b[b_pos]
                        const bool eA = hasA && bt == va[c], eB = hasB && bt == vb[c];
                        seenA[c] = seenA[c] || (below && eA);
                        seenB[c] = seenB[c] || (below && eB);
                        if (kt == NMZ_EDIT_INS && kind[c] == NMZ_EDIT_INS && below && eB) ++rank[c];
                    }
                }
            }
            // ---- the partner: (opposite kind, value, rank)
            bool anyDel = false, anyIns = false;
#pragma unroll
            for (uint32_t c = 0; c < MW_C; ++c) {
                const uint32_t s = tid + MW_THREADS * c;
                if (s < d) s_rank[s] = rank[c];
                anyDel = anyDel || kind[c] == NMZ_EDIT_DEL;
                anyIns = anyIns || kind[c] == NMZ_EDIT_INS;
            }
            const int hasDel = __syncthreads_or(anyDel ? 1 : 0);  // the ranks are in LDS behind these barriers
            const int hasIns = __syncthreads_or(anyIns ? 1 : 0);
            if (hasDel && hasIns) {
                for (uint32_t t = 0; t < d; ++t) {
                    const uint32_t kt = s_kind[t];
                    if (kt != NMZ_EDIT_DEL && kt != NMZ_EDIT_INS) continue;
                    const uint32_t rt = s_rank[t];
                    const uint64_t vt = kt == NMZ_EDIT_DEL ? s_va[t] : s_vb[t];
                    const uint32_t want = kt == NMZ_EDIT_DEL ? NMZ_EDIT_INS : NMZ_EDIT_DEL;
#pragma unroll
                    for (uint32_t c = 0; c < MW_C; ++c) {
                        const uint64_t mine = kt == NMZ_EDIT_DEL ? vb[c] : va[c];
                        if (kind[c] == want && mine == vt && rank[c] == rt) pr[c] = t;
                    }
                }
            }
            // ---- the tally
#pragma unroll
            for (uint32_t c = 0; c < MW_C; ++c) {
                const uint32_t s = tid + MW_THREADS * c;
                const bool hasA = kind[c] == NMZ_EDIT_SUB || kind[c] == NMZ_EDIT_DEL;
                const bool hasB = kind[c] == NMZ_EDIT_SUB || kind[c] == NMZ_EDIT_INS;
                const uint32_t pb = pr[c] != NMZ_NONE ? s_bp[pr[c]] : bp[c];  // the partner's b_pos
                const uint64_t iA =
                    hasA ? (LDS ? mv_find(s_tab, g.n_usym, va[c]) : mv_find(g.usym, g.n_usym, va[c])) : MV_MISS;
                const uint64_t iB =
                    hasB ? (LDS ? mv_find(s_tab, g.n_usym, vb[c]) : mv_find(g.usym, g.n_usym, vb[c])) : MV_MISS;
                n_unknown += (hasA && iA == MV_MISS ? 1u : 0u) + (hasB && iB == MV_MISS ? 1u : 0u);
                if (iA != MV_MISS) {
                    nmz_move_counts *cnt = g.counts + iA;
                    if (kind[c] == NMZ_EDIT_SUB) {
                        atomicAdd(&cnt->sub_from, 1u);
                    } else if (pr[c] == NMZ_NONE) {
                        atomicAdd(&cnt->dropped, 1u);
                    } else {  // the DEL slot counts the move
                        const unsigned long long span = pb > bp[c] ? pb - bp[c] : bp[c] - pb;
                        if (pr[c] > s) {
                            atomicAdd(&cnt->later, 1u);
                            atomicAdd((unsigned long long *)&cnt->span_later, span);
                        } else {
                            atomicAdd(&cnt->earlier, 1u);
                            atomicAdd((unsigned long long *)&cnt->span_earlier, span);
                        }
                    }
                    if (!seenA[c]) atomicAdd(&cnt->n_pairs, 1u);
                }
                if (iB != MV_MISS) {
                    nmz_move_counts *cnt = g.counts + iB;
                    if (kind[c] == NMZ_EDIT_SUB) {
                        atomicAdd(&cnt->sub_to, 1u);
                    } else if (pr[c] == NMZ_NONE) {
                        atomicAdd(&cnt->extra, 1u);
                    }
                    if (!seenB[c] && !(hasA && va[c] == vb[c])) atomicAdd(&cnt->n_pairs, 1u);
                }
            }
        }
        if (g.partner) {
#pragma unroll
            for (uint32_t c = 0; c < MW_C; ++c) {
                const uint32_t s = tid + MW_THREADS * c;
                if (s < band) g.partner[p * band + s] = pr[c];
            }
        }
    }
    // info: the threads' sums meet in LDS, and the workgroup adds each nonzero word once
    if (tid == 0) {
        s_info[0] = n_scripts;
        s_info[1] = n_beyond;
        s_info[2] = n_ops;
    }
    __syncthreads();
    if (n_unknown) atomicAdd(&s_info[3], (unsigned long long)n_unknown);
    __syncthreads();
    if (tid < 4 && s_info[tid]) atomicAdd((unsigned long long *)g.info + tid, s_info[tid]);
}

// K9w's launch behind its argument checks and the clear; a band <= 64 goes to K9. The caller holds the context.
int moves_wide_enqueue(nmz_ctx *ctx, hipStream_t st, const MvArgs &a, int accumulate) {
    NMZ_TRY(aw_band(a.band));
    if (a.band <= NMZ_ALIGN_MAX_BAND) return moves_enqueue(ctx, st, a, accumulate);
    NMZ_CHECK(a.n_pairs * (uint64_t)a.band < (1ull << 32) && (a.band == 0 || a.n_pairs < (1ull << 32)),
              "n_pairs * band = " + std::to_string(a.n_pairs) + " * " + std::to_string(a.band) + " must stay below "
              "2^32: a uint32 counter could wrap");
    NMZ_CHECK(a.n_usym == 0 || (a.usym && a.counts), "d_usym or d_counts is NULL");
    NMZ_CHECK(a.info != nullptr, "d_info is NULL");
    NMZ_CHECK(a.n_usym <= SIZE_MAX / sizeof(nmz_move_counts), "n_usym does not fit the counters");
    if (!accumulate) {
        if (a.n_usym) NMZ_HIP(hipMemsetAsync(a.counts, 0, (size_t)a.n_usym * sizeof(nmz_move_counts), st));
        NMZ_HIP(hipMemsetAsync(a.info, 0, sizeof(nmz_move_info), st));
    }
    if (a.n_pairs == 0) return NMZ_OK;
    NMZ_CHECK(a.off && a.pairs && a.dist, "d_off, d_pairs or d_dist is NULL");
    NMZ_CHECK(a.ops != nullptr, "d_ops is NULL");
    const bool lds = a.n_usym <= MV_LDS_SYMS;
    const unsigned blocks = (unsigned)std::min<uint64_t>(
        a.n_pairs, (uint64_t)std::max(ctx->n_cu, 1) * (lds ? MW_BLOCKS_PER_CU_LDS : MW_BLOCKS_PER_CU_GLOBAL));
    KernelTimer kt(ctx, st, "script_moves_wide");
    if (lds)
        hipLaunchKernelGGL(k_script_moves_wide<true>, dim3(blocks), dim3(MW_THREADS), 0, st, a);
    else
        hipLaunchKernelGGL(k_script_moves_wide<false>, dim3(blocks), dim3(MW_THREADS), 0, st, a);
    if (hipGetLastError() != hipSuccess) return fail(NMZ_EHIP, "k_script_moves_wide launch failed");
    return NMZ_OK;
}

}  // namespace nmz

using namespace nmz;

extern "C" {

// The whole profile on the calling thread (historystorage.go:50-51, naive.go:199-213, 235-257):
// nmz_move_profile_host's body behind the wide band check. Nothing shared with the kernels.
int nmz_move_profile_wide_host(const uint64_t *off, const uint64_t *sym, uint32_t n_traces, const uint32_t *pairs,
                               uint64_t n_pairs, uint32_t band, const uint32_t *dist, const nmz_edit_op *ops,
                               const uint64_t *usym, uint64_t n_usym, uint32_t *partner, nmz_move_counts *counts,
                               nmz_move_info *info) {
    return moves_profile_host(aw_band, aw_validate, off, sym, n_traces, pairs, n_pairs, band, dist, ops, usym, n_usym,
                              partner, counts, info);
}

int nmz_move_profile_wide_dev(nmz_ctx *ctx, const uint64_t *d_off, const uint64_t *d_sym, const uint32_t *d_pairs,
                              uint64_t n_pairs, uint32_t band, const uint32_t *d_dist, const nmz_edit_op *d_ops,
                              const uint64_t *d_usym, uint64_t n_usym, uint32_t *d_partner, nmz_move_counts *d_counts,
                              nmz_move_info *d_info, int accumulate, void *stream) {
    NMZ_CHECK(ctx != nullptr, "ctx is NULL");
    CtxGuard g(ctx);
    NMZ_TRY(g.rc);
    const MvArgs a{d_off, d_sym, d_pairs, n_pairs, band, d_dist, d_ops, d_usym, n_usym, d_partner, d_counts, d_info};
    return moves_wide_enqueue(ctx, stream ? (hipStream_t)stream : ctx->stream, a, accumulate);
}

int nmz_move_profile_wide(nmz_ctx *ctx, const uint64_t *off, const uint64_t *sym, uint32_t n_traces,
                          const uint32_t *pairs, uint64_t n_pairs, uint32_t band, const uint32_t *dist,
                          const nmz_edit_op *ops, const uint64_t *usym, uint64_t n_usym, uint32_t *partner,
                          nmz_move_counts *counts, nmz_move_info *info) {
    // the arguments first: they are checked without a device
    uint64_t max_len = 0;
    NMZ_TRY(moves_validate(aw_band, aw_validate, off, sym, n_traces, pairs, n_pairs, band, dist, ops, true, usym, n_usym,
                           counts, info, &max_len));
    if (n_pairs == 0) {  // all zero: no device either
        moves_zero(counts, n_usym, info);
        return NMZ_OK;
    }
    NMZ_CHECK(ctx != nullptr, "ctx is NULL");
    CtxGuard g(ctx);
    NMZ_TRY(g.rc);
    HostCall call(ctx);  // owns no plan: call.work holds the buffers, drained before they go back to the pool
    hipStream_t st = ctx->stream;
    const uint64_t total = off[n_traces];
    const size_t n_slots = (size_t)n_pairs * band;
    uint64_t *d_off, *d_sym, *d_usym;
    uint32_t *d_pairs, *d_dist, *d_partner;
    nmz_edit_op *d_ops;
    nmz_move_counts *d_counts;
    nmz_move_info *d_info;
    ScratchLayout lay;
    lay.add(&d_off, n_traces + 1).add(&d_sym, total + 1).add(&d_pairs, 2 * n_pairs).add(&d_dist, n_pairs);
    lay.add(&d_ops, n_slots + 1).add(&d_usym, n_usym + 1).add(&d_partner, n_slots + 1).add(&d_counts, n_usym + 1);
    lay.add(&d_info, 1);
    NMZ_TRY(lay.bind(call.work));
    NMZ_TRY(upload_csr(d_off, d_sym, off, sym, n_traces, st));
    NMZ_TRY(copy_h2d(d_pairs, pairs, 2 * n_pairs, st));
    NMZ_TRY(copy_h2d(d_dist, dist, n_pairs, st));
    NMZ_TRY(copy_h2d(d_ops, ops, n_slots, st));
    NMZ_TRY(copy_h2d(d_usym, usym, n_usym, st));
    const MvArgs a{d_off, d_sym, d_pairs, n_pairs, band, d_dist, d_ops, d_usym, n_usym, partner ? d_partner : nullptr,
                   d_counts, d_info};
    NMZ_TRY(moves_wide_enqueue(ctx, st, a, 0));
    if (partner) NMZ_TRY(copy_d2h(partner, d_partner, n_slots, st));
    NMZ_TRY(copy_d2h(counts, d_counts, n_usym, st));
    NMZ_TRY(copy_d2h(info, d_info, 1, st));
    return call.done();
}

int nmz_ed_diff_profile_wide(nmz_ctx *ctx, const uint64_t *off, const uint64_t *sym, uint32_t n_traces,
                             const uint32_t *pairs, uint64_t n_pairs, uint32_t band, const uint64_t *usym,
                             uint64_t n_usym, uint32_t *dist, nmz_move_counts *counts, nmz_move_info *info) {
    // the arguments first: they are checked without a device
    uint64_t max_len = 0, slot_words = 0;
    NMZ_TRY(moves_validate(aw_band, aw_validate, off, sym, n_traces, pairs, n_pairs, band, dist, nullptr, false, usym,
                           n_usym, counts, info, &max_len));
    if (n_pairs == 0) {  // all zero: no device either
        moves_zero(counts, n_usym, info);
        return NMZ_OK;
    }
    NMZ_TRY(aw_shape(band, max_len, &slot_words));
    NMZ_CHECK(ctx != nullptr, "ctx is NULL");
    CtxGuard g(ctx);
    NMZ_TRY(g.rc);
    HostCall call(ctx);
    nmz_ed_align_wide_plan *plan = nullptr;
    NMZ_TRY(aw_plan_create_locked(ctx, band, max_len, slot_words, &plan));
    call.own_plan<aw_plan_destroy_locked>(plan);
    hipStream_t st = ctx->stream;
    const uint64_t total = off[n_traces];
    const size_t n_slots = (size_t)n_pairs * band;
    uint64_t *d_off, *d_sym, *d_usym;
    uint32_t *d_pairs, *d_dist;
    nmz_edit_op *d_ops;
    nmz_move_counts *d_counts;
    nmz_move_info *d_info;
    ScratchLayout lay;
    lay.add(&d_off, n_traces + 1).add(&d_sym, total + 1).add(&d_pairs, 2 * n_pairs).add(&d_dist, n_pairs);
    lay.add(&d_ops, n_slots + 1).add(&d_usym, n_usym + 1).add(&d_counts, n_usym + 1).add(&d_info, 1);
    NMZ_TRY(lay.bind(call.work));
    NMZ_TRY(upload_csr(d_off, d_sym, off, sym, n_traces, st));
    NMZ_TRY(copy_h2d(d_pairs, pairs, 2 * n_pairs, st));
    NMZ_TRY(copy_h2d(d_usym, usym, n_usym, st));
    NMZ_TRY(aw_enqueue(plan, st, d_off, d_sym, d_pairs, n_pairs, d_dist, d_ops));
    const MvArgs a{d_off, d_sym, d_pairs, n_pairs, band, d_dist, d_ops, d_usym, n_usym, nullptr, d_counts, d_info};
    NMZ_TRY(moves_wide_enqueue(ctx, st, a, 0));
    if (dist) NMZ_TRY(copy_d2h(dist, d_dist, n_pairs, st));
    NMZ_TRY(copy_d2h(counts, d_counts, n_usym, st));
    NMZ_TRY(copy_d2h(info, d_info, 1, st));
    return call.done();
}

}  // extern "C"
