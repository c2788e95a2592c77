// K11w -- PO k-NN search over bands wider than one wave holds: 64 < w <= 1,024
// (historystorage/historystorage.go:50-51 is the search interface this extends, naive/naive.go:235-257 the
// reference's equality search, cli/tools/visualize.go:62-136 createTracesPerEntity / tracesEqualInPO: d == 0 <=>
// tracesEqualInPO).
//
// The semantics are K11's (ed_po_knn.hip; DESIGN.md section 2, "PO k-NN search") word for word with 0 <= band <=
// 1,024. The plan, the projection, the profiles, the guard, the init and the fill are K11's and are not repeated
// here: pk_enqueue (ed_po_knn.hip) launches this kernel in K11b's place when the plan's band is above 64.
//
// k_po_knn_wide<CMAX>: K11b one level up, as K8w is K8 one level up. A persistent
// workgroup of 256 threads (4 waves) takes K11b's work items -- (query, block of 64 stored traces, part p of P) --
// from the one item counter.
//   item    wave 0 fetches the item (lane 0's atomic) and runs K11b's filter on it, a lane per candidate, then
//           publishes {item, the survivors' ballot, the number of eligible candidates} in LDS behind a barrier. One
//           wave filters and the others wait: four redundant filters would read each candidate's 256 bytes four
//           times for nothing (a part already repeats its block's filter), and a published ballot makes the survivor
//           set, the part test and everything after them uniform over the workgroup by construction.
//   pair    as in K11b, every wave for itself (the rows of projected offsets are read-only while the kernel runs, so
//           the four waves hold the same scalars): the exact sum of ||q|g| - |c|g||, then the entities where either
//           side is not empty, ascending, each against the budget r = w - (the sum so far).
//   DP      per entity, distance only (AlignNoMoves), over ed_align_dev.h's pieces with K8w's exchange: the cells
//           blocked over the 256 threads, one __syncthreads() per row, double-buffered records {wave minimum, first
//           cell's t, liveness of the row before}; the cut-off comes one row late, against r. The entity's band is
//           clamped: w_g = min(r, max(n_g, m_g)). Lev <= max(n, m) always, so the clamp is exact, and it lays 257
//           cells per row where 2,049 would be laid for 128-event projections at band 1,024. C, the cells per thread,
//           follows from w_g by aw_cells (C = 1, 2, 3, 5, 9 for w_g <= 127, 255, 383, 639, 1,024) through a uniform
//           switch over the instantiations C <= CMAX; CMAX = aw_cells(the plan's band). NMZ_PO_KNN_OPT_FULL_BAND lays
//           every entity out for the plan's band at C = CMAX instead (A/B and tests; the same lists).
//           An entity ends the pair at w + 1 when ||n| - |m|| > r, when a row has no cell <= r, or when its result
//           exceeds r: Lev_g > r => the sum > w, K11b's argument.
//   lists   thread 0 puts an in-band result into the query's list by knn_insert; k_po_knn_fill completes the lists.
// Every barrier sits in control flow that depends only on values read from LDS behind a barrier (the item, the
// ballot, a row's records, the final cell) or on the read-only offsets, so it is uniform over the workgroup. No
// spin, no wait on another workgroup. Atomics: the lists', the counters' and the item counter's. No scratch;
// nothing is allocated per launch.
// Counters: K11's four, then the entity steps run at C = 1, 2, 3, 5, 9 (words 4 .. 8).
#include <algorithm>
#include <string>

#include "ed_align_dev.h"
#include "ed_knn_dev.h"
#include "ed_po_knn.h"
#include "nmz_common.h"
#include "nmz_internal.h"

namespace nmz {

static_assert(NMZ_PO_KNN_WIDE_MAX_BAND == NMZ_ALIGN_WIDE_MAX_BAND, "aw_cells covers the band: C = 9 holds 2 * 1024 + 1");
static_assert(PKW_NSTEPS == 5, "one step counter per C in {1, 2, 3, 5, 9}");

// what wave 0 publishes per item
struct PkwItem {
    unsigned long long item;
    uint64_t todo;     // the block's survivors
    uint32_t n_valid;  // the block's eligible candidates
    uint32_t pad;
};

// Lev(a, b) when it is <= r, anything > r otherwise; |n - m| <= min(r, wl), and wl >= min(r, max(n, m)). The band's
// cells are laid out for wl over the workgroup, C = aw_cells(wl) or more. Every thread of the workgroup calls it.
template <int C>
__device__ __forceinline__ uint32_t pkw_lev(const uint64_t *__restrict__ a, int64_t n, const uint64_t *__restrict__ b,
                                            int64_t m, int32_t wl, int32_t r, uint64_t *s_a, uint64_t *s_b,
                                            AwRec (*s_rec)[AW_WAVES + 1], int32_t *s_fin, uint32_t tid) {
    // row 0 alone: D[0][m] = m <= r. (Also what keeps two writes of s_fin a staging barrier apart.)
    if (n == 0) return (uint32_t)min(m, (int64_t)r + 1);
    const uint32_t lane = tid & 63, wv = tid >> 6;
    const int32_t W2 = 2 * wl;
    const int32_t d0 = (int32_t)tid * C;            // this thread's first cell
    const int32_t dn = (int32_t)(wv + 1) * 64 * C;  // the next wave's first cell
    int32_t prev[C];
    AlignNoMoves distance_only;
    align_row0<C>(prev, d0, wl, m);
    int32_t edge = (dn <= W2 && dn >= wl && (int64_t)dn - wl <= m) ? dn - wl : ALIGN_INF;  // row 0's cell dn
    bool live_prev = true;
    for (int64_t i0 = 0; i0 < n; i0 += ALIGN_ROWS) {
        const int32_t rows = (int32_t)min((int64_t)ALIGN_ROWS, n - i0);
        align_stage<uint32_t, AW_THREADS>(s_a, s_b, a, n, b, m, i0, wl, tid);
        for (int32_t rr = 1; rr <= rows; ++rr) {
            const int par = rr & 1;
            const uint64_t ai = s_a[rr - 1];
            int32_t nxt = align_dpp<DPP_WAVE_SHL1>(ALIGN_INF, prev[0]);  // the next thread's first cell
            nxt = lane == 63 ? edge : nxt;
            int32_t t[C], lp[C];
            bool valid[C];
            align_row_candidates<C>(prev, nxt, ai, s_b, rr, d0, wl, m, i0 + rr, t, valid, lp, distance_only);
            const int32_t incl = align_scan_min(lp[C - 1]);
            const int32_t below = align_dpp<DPP_WAVE_SHR1>(ALIGN_INF, incl);  // the lanes below, this wave
            if (lane == 63) s_rec[par][wv].wmin = incl;
            if (lane == 0) {
                s_rec[par][wv].t0 = valid[0] ? min(t[0], ALIGN_INF) : -1;
                s_rec[par][wv].live = live_prev ? 1 : 0;
            }
            __syncthreads();  // the row's one barrier
            const AwRec r0 = s_rec[par][0], r1 = s_rec[par][1], r2 = s_rec[par][2], r3 = s_rec[par][3];
            // the row before had no cell <= r: its minimum, and so the entity's distance, has passed the budget
            if ((r0.live | r1.live | r2.live | r3.live) == 0) return (uint32_t)r + 1;
            int32_t wbelow = ALIGN_INF;  // the waves below this one
            wbelow = wv > 0 ? min(wbelow, r0.wmin) : wbelow;
            wbelow = wv > 1 ? min(wbelow, r1.wmin) : wbelow;
            wbelow = wv > 2 ? min(wbelow, r2.wmin) : wbelow;
            const int32_t own = wv == 0 ? r0.wmin : (wv == 1 ? r1.wmin : (wv == 2 ? r2.wmin : r3.wmin));
            const int32_t nt0 = s_rec[par][wv + 1].t0;
            edge = nt0 < 0 ? ALIGN_INF : min(min(nt0, dn + min(wbelow, own)), ALIGN_INF);  // this row's cell dn
            const int32_t excl = min(below, wbelow);
            const bool live = align_row_close<C>(prev, valid, lp, excl, d0, r, distance_only);
            live_prev = __ballot(live) != 0;
        }
    }
    const int32_t df = (int32_t)(m - n) + wl;  // in [0, 2 wl]
    if ((int32_t)tid == df / C) *s_fin = align_final_cell<C>(prev, df);
    __syncthreads();
    return (uint32_t)min(*s_fin, r + 1);
}

// the uniform switch over the instantiations C <= CMAX
template <int CMAX>
__device__ __forceinline__ uint32_t pkw_lev_cells(int C, const uint64_t *__restrict__ a, int64_t n,
                                                  const uint64_t *__restrict__ b, int64_t m, int32_t wl, int32_t r,
                                                  uint64_t *s_a, uint64_t *s_b, AwRec (*s_rec)[AW_WAVES + 1],
                                                  int32_t *s_fin, uint32_t tid) {
    if constexpr (CMAX >= 9) {
        if (C == 9) return pkw_lev<9>(a, n, b, m, wl, r, s_a, s_b, s_rec, s_fin, tid);
    }
    if constexpr (CMAX >= 5) {
        if (C == 5) return pkw_lev<5>(a, n, b, m, wl, r, s_a, s_b, s_rec, s_fin, tid);
    }
    if constexpr (CMAX >= 3) {
        if (C == 3) return pkw_lev<3>(a, n, b, m, wl, r, s_a, s_b, s_rec, s_fin, tid);
    }
    if constexpr (CMAX >= 2) {
        if (C == 2) return pkw_lev<2>(a, n, b, m, wl, r, s_a, s_b, s_rec, s_fin, tid);
    }
    return pkw_lev<1>(a, n, b, m, wl, r, s_a, s_b, s_rec, s_fin, tid);
}

template <int CMAX>
__global__ __launch_bounds__(AW_THREADS) void k_po_knn_wide(const PkArgs g) {
    constexpr int WMAX = aw_wmax(CMAX);
    __shared__ uint64_t s_a[ALIGN_ROWS];
    __shared__ uint64_t s_b[ALIGN_ROWS + 2 * WMAX];
    __shared__ AwRec s_rec[2][AW_WAVES + 1];  // [.][AW_WAVES]: "the wave after the last", never a cell
    __shared__ PkwItem s_it;
    __shared__ int32_t s_fin;
    if (*g.over) return;
    const uint32_t tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const uint32_t w = g.w, G = g.G;
    if (tid < 2) s_rec[tid][AW_WAVES] = AwRec{ALIGN_INF, -1, 0, 0};
    uint64_t n_filter = 0, n_len = 0, n_dp = 0, n_in = 0;    // uniform over the workgroup
    uint64_t st1 = 0, st2 = 0, st3 = 0, st5 = 0, st9 = 0;    // entity steps at C = 1, 2, 3, 5, 9
    for (;;) {
        __syncthreads();  // the item before: its reads of s_it (and, the first time, s_rec's last column)
        if (wv == 0) {    // no barrier inside
            unsigned long long item = 0;
            if (lane == 0) item = atomicAdd(g.next, 1ull);
            item = pk_lane64(item, 0);
            uint64_t todo = 0;
            uint32_t n_valid = 0;
            if (item < g.n_items) {
                const uint64_t blk = item / g.parts;
                const uint32_t q = (uint32_t)(blk / g.NB);
                const uint32_t cb = (uint32_t)(blk - (uint64_t)q * g.NB);
                const uint32_t self = g.q_self ? g.q_self[q] : NMZ_NONE;
                const uint32_t cand = cb * 64 + lane;
                const bool valid = cand < g.N && cand != self;
                bool survive = valid;
                if (!g.no_filter) {
                    const uint32_t *__restrict__ qp = g.q_prof + (uint64_t)q * PK_PROF_WORDS;  // uniform
                    const uint4 *__restrict__ cp =
                        (const uint4 *)(g.prof + (uint64_t)(valid ? cand : 0) * PK_PROF_WORDS);
                    const bool passes = pk_filter_passes(qp, cp, w);  // every lane: no branch round the loads
                    survive = valid && passes;
                }
                todo = __ballot(survive);
                n_valid = (uint32_t)__popcll(__ballot(valid));
            }
            if (lane == 0) s_it = PkwItem{item, todo, n_valid, 0};
        }
        __syncthreads();
        const unsigned long long item = s_it.item;
        if (item >= g.n_items) break;
        uint64_t todo = s_it.todo;
        const uint32_t n_valid = s_it.n_valid;
        const uint64_t blk = item / g.parts;
        const uint32_t part = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(item - blk * g.parts));
        const uint32_t q = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(blk / g.NB));
        const uint32_t cb = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(blk - (uint64_t)q * g.NB));
        if (part == 0) n_filter += n_valid - (uint32_t)__popcll(todo);
        uint32_t nth = 0;  // of the block's survivors
        const uint64_t *__restrict__ qrow = g.q_poff + (uint64_t)q * G;
        // ---- the DP: the workgroup per surviving pair
        while (todo) {  // uniform
            const uint32_t bit = (uint32_t)__builtin_amdgcn_readfirstlane(__ffsll((unsigned long long)todo) - 1);
            todo &= todo - 1;
            if (nth++ % g.parts != part) continue;  // another part's pair
            const uint32_t c = cb * 64 + bit;
            const uint64_t *__restrict__ crow = g.poff + (uint64_t)c * G;
            // the exact sum of the entities' length differences, every wave for itself
            uint32_t lsum = 0;
            for (uint32_t g0 = 0; g0 < G && lsum <= w; g0 += 64) {
                const uint32_t e = g0 + lane;
                uint32_t diff = 0;
                if (e < G) {
                    const uint64_t la = qrow[e + 1] - qrow[e], lb = crow[e + 1] - crow[e];
                    diff = (uint32_t)min(la > lb ? la - lb : lb - la, (uint64_t)w + 1);
                }
                // the per-lane min(diff, w + 1) keeps the sum within 32 bits at w = 1,024: <= 64 * 1,025 per chunk,
                // <= 16 chunks (NMZ_PO_MAX_ENTITIES = 1,024), so <= 1,049,600
                lsum += pk_wave_sum(diff);
            }
            if (lsum > w) {
                ++n_len;
                continue;
            }
            ++n_dp;
            uint32_t sum = 0;
            bool beyond = false;
            for (uint32_t g0 = 0; g0 < G && !beyond; g0 += 64) {
                const uint32_t e = g0 + lane;
                uint64_t qlo = 0, qhi = 0, clo = 0, chi = 0;
                if (e < G) qlo = qrow[e], qhi = qrow[e + 1], clo = crow[e], chi = crow[e + 1];
                uint64_t ents = __ballot(qhi > qlo || chi > clo);
                while (ents) {  // uniform, ascending entity
                    const int src = __builtin_amdgcn_readfirstlane(__ffsll((unsigned long long)ents) - 1);
                    ents &= ents - 1;
                    const uint64_t a0 = pk_lane64(qlo, src), a1 = pk_lane64(qhi, src);
                    const uint64_t b0 = pk_lane64(clo, src), b1 = pk_lane64(chi, src);
                    const int64_t n = (int64_t)(a1 - a0), m = (int64_t)(b1 - b0);
                    const int32_t r = (int32_t)(w - sum);  // the budget: what the entities before have left
                    if ((n > m ? n - m : m - n) > (int64_t)r) {
                        beyond = true;
                        break;
                    }
                    // the entity's band: Lev <= max(n, m), so no cell beyond min(r, max(n, m)) is needed
                    const int32_t wl = g.full_band ? (int32_t)w : (int32_t)min((int64_t)r, max(n, m));
                    const int C = g.full_band ? CMAX : aw_cells((uint32_t)wl);
                    st1 += C == 1, st2 += C == 2, st3 += C == 3, st5 += C == 5, st9 += C == 9;
                    const uint32_t d = pkw_lev_cells<CMAX>(C, g.q_psym + a0, n, g.psym + b0, m, wl, r, s_a, s_b, s_rec,
                                                           &s_fin, tid);
                    if (d > (uint32_t)r) {
                        beyond = true;
                        break;
                    }
                    sum += d;
                }
            }
            if (!beyond) {
                ++n_in;
                if (tid == 0) knn_insert(g.knn + (uint64_t)q * g.k, g.k, ((uint64_t)sum << 32) | c);
            }
        }
    }
    if (tid < PKW_NCOUNTERS) {
        const uint64_t lo = tid == 0 ? n_filter : (tid == 1 ? n_len : (tid == 2 ? n_dp : n_in));
        const uint64_t hi = tid == 4 ? st1 : (tid == 5 ? st2 : (tid == 6 ? st3 : (tid == 7 ? st5 : st9)));
        const uint64_t v = tid < PK_NCOUNTERS ? lo : hi;
        if (v) atomicAdd((unsigned long long *)&g.counters[(blockIdx.x % ED_CNT_STRIPES) * ED_CNT_LINE + tid],
                         (unsigned long long)v);
    }
}

// The workgroups a CU holds at once (`make resources`): a workgroup puts one wave on each
// SIMD, so the waves per SIMD that the registers allow -- 115, 156, 138, 169 and 239 VGPRs give 4, 3, 3, 2 and 2 --
// are the workgroups per CU; 160 KiB of LDS over 3,248 .. 17,600 bytes per workgroup would hold 9 or more.
static uint32_t pkw_wgs_per_cu(int cmax) { return cmax == 1 ? 4 : (cmax <= 3 ? 3 : 2); }

uint64_t pkw_resident(const nmz_ctx *ctx, uint32_t band) {
    return (uint64_t)std::max(ctx->n_cu, 1) * pkw_wgs_per_cu(aw_cells(band));
}

int pkw_launch(nmz_ctx *ctx, hipStream_t st, const PkArgs &a, unsigned blocks) {
    NMZ_CHECK(a.w > NMZ_PO_KNN_MAX_BAND && a.w <= NMZ_PO_KNN_WIDE_MAX_BAND,
              "k_po_knn_wide serves bands 65 .. 1024, not " + std::to_string(a.w));
    KernelTimer kt(ctx, st, "po_knn_wide");
    switch (aw_cells(a.w)) {
        case 1: hipLaunchKernelGGL(k_po_knn_wide<1>, dim3(blocks), dim3(AW_THREADS), 0, st, a); break;
        case 2: hipLaunchKernelGGL(k_po_knn_wide<2>, dim3(blocks), dim3(AW_THREADS), 0, st, a); break;
        case 3: hipLaunchKernelGGL(k_po_knn_wide<3>, dim3(blocks), dim3(AW_THREADS), 0, st, a); break;
        case 5: hipLaunchKernelGGL(k_po_knn_wide<5>, dim3(blocks), dim3(AW_THREADS), 0, st, a); break;
        default: hipLaunchKernelGGL(k_po_knn_wide<9>, dim3(blocks), dim3(AW_THREADS), 0, st, a); break;
    }
    if (hipGetLastError() != hipSuccess) return fail(NMZ_EHIP, "k_po_knn_wide launch failed");
    return NMZ_OK;
}

}  // namespace nmz
