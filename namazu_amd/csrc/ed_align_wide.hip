// K8w -- edit scripts for trace pairs over bands wider than one wave holds: 64 < w <= 1,024
// (historystorage/historystorage.go:50-51 is the search interface this extends, naive/naive.go:235-257 the
// reference's equality search, util/trace/trace.go:29-31 SingleTrace.Equals: an empty script <=> Equals).
//
// The semantics are K8's (ed_align.hip; DESIGN.md section 2, "Edit scripts") word for word: dist = min(Lev, w + 1)
// and, for dist <= w, the canonical alignment -- diagonal, then up, then left -- in forward order, `band` slots per
// pair, sentinels behind the ops. The nmz_ed_align_wide_* entry points take every band 0 .. 1,024; a band <= 64 runs
// k_ed_align through a narrow plan that the wide plan owns, so it gives the narrow entry points' bytes.
//
// k_ed_align_wide<C>: K8 one level up, over the same pieces (ed_align_dev.h). One
// workgroup of 256 threads (4 waves) per pair, grid-striding over the pairs; it owns one history slot of the plan.
// The band's 2w + 1 cells of a row (cell d <-> j = i + d - w) lie blocked over the threads, C in {1, 2, 3, 5, 9}
// consecutive cells per thread (w <= 127, 255, 383, 639, 1,024), in named registers. Per row, ONE workgroup barrier:
//   1. t[d] = min(prev[d] + (a[i-1] != b[j-1]), prev[d + 1] + 1). "Up" of a thread's last cell is the next
//      thread's first: a DPP lane shift, and for lane 63 the next wave's first cell, which this wave worked out
//      itself at the end of the row before (step 4). a and the row block's window of b are staged in LDS by
//      coalesced loads once per 64 rows.
//   2. the closure D[d] = d + prefixmin(t[d'] - d'): a serial pass over the thread's cells, K8's 6-step DPP scan of
//      the lanes' minima, then the waves' minima through LDS. Each wave publishes {its minimum, its first cell's t,
//      whether the row before had a cell <= w}; the barrier; each wave reads the four records.
//   3. two ballots per cell column c and wave, the same 2 bits per cell as K8; lane 0 puts the pair of words in the
//      LDS image of the row block ([row][c][wave]{diag, low}); one coalesced copy per block writes it to the slot.
//   4. the next row's lane-63 "up" for wave v is cell d = 64 C (v + 1): min(its t, d + the minimum over waves
//      <= v), both known after the barrier. So no second barrier is needed for it.
//   The cut-off lags a row: a row's liveness travels with the next row's record, and a row without a cell <= w
//   ends the pair at dist = w + 1 one row later (a dead row's successors are dead, and the last row needs no check:
//   its own cell gives dist). The records are double-buffered by row parity, which one barrier per row makes safe.
// The walk is K8's, written out here as there: the history a 64-row block at a time into LDS (the newest block is still there), LDS reads
// only; every thread takes the same steps, thread 0 puts the t-th op found into slot dist - 1 - t of an LDS array
// that was filled with sentinels, and one coalesced pass stores the pair's `band` slots. No scratch, no atomics;
// nothing is allocated per launch.
#include <algorithm>
#include <new>
#include <string>
#include <vector>

#include "ed_align_dev.h"
#include "ed_plan.h"
#include "nmz_common.h"
#include "nmz_internal.h"

namespace nmz {

// AW_THREADS, AW_WAVES, aw_wmax, aw_cells and AwRec: ed_align_dev.h, shared with K11w
static_assert(NMZ_ALIGN_WIDE_MAX_BAND == 1024, "C = 9 cells per thread cover 2 * 1024 + 1 cells");

// the workgroups a CU holds at once: registers give 8, 7, 6, 5 and 3 waves per SIMD, one
// per workgroup; 160 KiB of LDS give 5 workgroups at C = 5 (31,896 bytes each) and 2 at C = 9 (54,440)
static uint32_t aw_slots_per_cu(int C) { return C == 1 ? 8 : (C == 2 ? 7 : (C == 3 ? 6 : (C == 5 ? 5 : 2))); }
static uint64_t aw_blocks(uint64_t max_len) { return std::max<uint64_t>(1, (max_len + ALIGN_ROWS - 1) / ALIGN_ROWS); }
// 64-bit words of one history block: [row][c][wave]{diag, low}
static uint64_t aw_block_words(int C) { return (uint64_t)ALIGN_ROWS * C * AW_WAVES * 2; }

struct AwArgs {
    const uint64_t *off, *sym;
    const uint32_t *pairs;
    uint64_t n_pairs;
    uint32_t band;
    uint64_t max_len;
    uint32_t *dist;
    nmz_edit_op *ops;
    uint64_t *hist;       // [slots][slot_words]
    uint64_t slot_words;  // blocks * 64 * C * 4 * 2
};

template <int C>
__global__ __launch_bounds__(AW_THREADS) void k_ed_align_wide(const AwArgs g) {
    constexpr int WMAX = aw_wmax(C);
    constexpr uint32_t BLK = ALIGN_ROWS * C * AW_WAVES;  // ulonglong2 records of one history block
    __shared__ uint64_t s_a[ALIGN_ROWS];
    __shared__ uint64_t s_b[ALIGN_ROWS + 2 * WMAX];  // the forward pass; the walk keeps the pair's ops over it
    __shared__ ulonglong2 s_h[BLK];
    __shared__ AwRec s_rec[2][AW_WAVES + 1];      // [.][AW_WAVES]: "the wave after the last", never a cell
    __shared__ int32_t s_fin;
    static_assert(sizeof(nmz_edit_op) * WMAX <= sizeof(uint64_t) * (ALIGN_ROWS + 2 * WMAX), "the ops fit s_b");
    nmz_edit_op *s_ops = reinterpret_cast<nmz_edit_op *>(s_b);
    const uint32_t tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int32_t w = (int32_t)g.band, W2 = 2 * w;
    const int32_t d0 = (int32_t)tid * C;             // this thread's first cell
    const int32_t dn = (int32_t)(wv + 1) * 64 * C;   // the next wave's first cell
    uint64_t *hist = g.hist + (uint64_t)blockIdx.x * g.slot_words;
    if (tid < 2) s_rec[tid][AW_WAVES] = AwRec{ALIGN_INF, -1, 0, 0};

    for (uint64_t p = blockIdx.x; p < g.n_pairs; p += gridDim.x) {
        const uint32_t ia = g.pairs[2 * p], ib = g.pairs[2 * p + 1];
        const uint64_t alo = g.off[ia], ahi = g.off[ia + 1], blo = g.off[ib], bhi = g.off[ib + 1];
        const uint64_t n64 = ahi > alo ? ahi - alo : 0, m64 = bhi > blo ? bhi - blo : 0;
        const uint64_t *__restrict__ a = g.sym + alo;
        const uint64_t *__restrict__ b = g.sym + blo;
        const int64_t n = (int64_t)n64, m = (int64_t)m64;
        uint32_t dist;
        int64_t loaded = -1;  // the history block that s_h holds

        if (n64 > g.max_len || m64 > g.max_len) {
            dist = NMZ_NONE;
        } else if ((n64 > m64 ? n64 - m64 : m64 - n64) > (uint64_t)w) {
            dist = (uint32_t)w + 1;  // the length filter
        } else {
            // ---- forward: row 0, then the rows in blocks of 64
            int32_t prev[C];
            align_row0<C>(prev, d0, w, m);
            int32_t edge = (dn <= W2 && dn >= w && (int64_t)dn - w <= m) ? dn - w : ALIGN_INF;  // row 0's cell dn
            bool alive = true, live_prev = true;
            for (int64_t i0 = 0; i0 < n && alive; i0 += ALIGN_ROWS) {
                const int32_t rows = (int32_t)min((int64_t)ALIGN_ROWS, n - i0);
                // its first barrier is also behind the previous block's reads of s_h and the previous pair's of s_ops;
                // the unsigned stride keeps the 8, 7, 6, 5 and 3 waves per SIMD that aw_slots_per_cu counts on
                align_stage<uint32_t, AW_THREADS>(s_a, s_b, a, n, b, m, i0, w, tid);
                for (int32_t r = 1; r <= rows; ++r) {
                    const int par = r & 1;
                    const uint64_t ai = s_a[r - 1];
                    int32_t nxt = align_dpp<DPP_WAVE_SHL1>(ALIGN_INF, prev[0]);  // the next thread's first cell
                    nxt = lane == 63 ? edge : nxt;
                    int32_t t[C], lp[C];
                    bool valid[C];
                    AlignMoves<C> mv;
                    align_row_candidates<C>(prev, nxt, ai, s_b, r, d0, w, m, i0 + r, t, valid, lp, mv);
                    const int32_t incl = align_scan_min(lp[C - 1]);
                    const int32_t below = align_dpp<DPP_WAVE_SHR1>(ALIGN_INF, incl);  // the lanes below, this wave
                    if (lane == 63) s_rec[par][wv].wmin = incl;
                    if (lane == 0) {
                        s_rec[par][wv].t0 = valid[0] ? min(t[0], ALIGN_INF) : -1;
                        s_rec[par][wv].live = live_prev ? 1 : 0;
                    }
                    __syncthreads();  // the row's one barrier
                    const AwRec r0 = s_rec[par][0], r1 = s_rec[par][1], r2 = s_rec[par][2], r3 = s_rec[par][3];
                    if ((r0.live | r1.live | r2.live | r3.live) == 0) {  // the row before had no cell <= w
                        alive = false;
                        break;
                    }
                    int32_t wbelow = ALIGN_INF;  // the waves below this one
                    wbelow = wv > 0 ? min(wbelow, r0.wmin) : wbelow;
                    wbelow = wv > 1 ? min(wbelow, r1.wmin) : wbelow;
                    wbelow = wv > 2 ? min(wbelow, r2.wmin) : wbelow;
                    const int32_t own = wv == 0 ? r0.wmin : (wv == 1 ? r1.wmin : (wv == 2 ? r2.wmin : r3.wmin));
                    const int32_t nt0 = s_rec[par][wv + 1].t0;
                    edge = nt0 < 0 ? ALIGN_INF : min(min(nt0, dn + min(wbelow, own)), ALIGN_INF);  // this row's cell dn
                    const int32_t excl = min(below, wbelow);
                    const bool live = align_row_close<C>(prev, valid, lp, excl, d0, w, mv);
#pragma unroll
                    for (int c = 0; c < C; ++c) {  // lane 0 puts the wave's words in the block's image
                        const uint64_t b1 = __ballot(mv.diag[c]), b0 = __ballot(mv.low[c]);
                        if (lane == 0) s_h[((uint32_t)(r - 1) * C + c) * AW_WAVES + wv] = make_ulonglong2(b1, b0);
                    }
                    live_prev = __ballot(live) != 0;
                }
                if (alive) {
                    __syncthreads();  // the block's image is whole
                    ulonglong2 *hb = reinterpret_cast<ulonglong2 *>(hist) + (uint64_t)(i0 / ALIGN_ROWS) * BLK;
                    for (uint32_t k = tid; k < (uint32_t)rows * C * AW_WAVES; k += AW_THREADS) hb[k] = s_h[k];
                    loaded = i0 / ALIGN_ROWS;
                }
            }
            if (!alive) {
                dist = (uint32_t)w + 1;
            } else {
                const int32_t df = (int32_t)(m - n) + w;  // in [0, 2 w] behind the length filter
                if ((int32_t)tid == df / C) s_fin = align_final_cell<C>(prev, df);
                __syncthreads();
                dist = (uint32_t)min(s_fin, w + 1);
            }
        }
        // ---- the pair's slots: sentinels, then the walk's ops over them
        __syncthreads();  // the forward pass is done with s_b (and the history stores precede the walk's loads)
        for (uint32_t s = tid; s < g.band; s += AW_THREADS) s_ops[s] = nmz_edit_op{NMZ_NONE, NMZ_NONE, NMZ_NONE};
        if (dist >= 1 && dist <= (uint32_t)w) {  // every thread takes the same steps
            int64_t i = n, j = m;
            uint32_t found = 0;
            __syncthreads();
            while (found < dist && (i | j) != 0) {
                uint32_t ka, kb, kk;
                if (i == 0) {
                    ka = 0, kb = (uint32_t)(j - 1), kk = NMZ_EDIT_INS;
                    --j;
                } else if (j == 0) {
                    ka = (uint32_t)(i - 1), kb = 0, kk = NMZ_EDIT_DEL;
                    --i;
                } else {
                    const int64_t blk = (i - 1) / ALIGN_ROWS;
                    if (blk != loaded) {
                        __syncthreads();
                        const ulonglong2 *hb = reinterpret_cast<const ulonglong2 *>(hist) + (uint64_t)blk * BLK;
                        for (uint32_t k = tid; k < BLK; k += AW_THREADS) s_h[k] = hb[k];
                        __syncthreads();
                        loaded = blk;
                    }
                    const int64_t d = j - i + w;
                    if (d < 0 || d > W2) break;  // cannot happen on an optimal path of cost <= w
                    const uint32_t r = (uint32_t)((i - 1) % ALIGN_ROWS), c = (uint32_t)d % C, th = (uint32_t)d / C;
                    const ulonglong2 h = s_h[(r * C + c) * AW_WAVES + (th >> 6)];
                    const uint32_t m1 = (uint32_t)(h.x >> (th & 63)) & 1u, m0 = (uint32_t)(h.y >> (th & 63)) & 1u;
                    if (m1) {
                        ka = (uint32_t)(i - 1), kb = (uint32_t)(j - 1), kk = m0 ? NMZ_EDIT_SUB : NMZ_NONE;
                        --i, --j;
                    } else if (m0) {
                        ka = (uint32_t)(i - 1), kb = (uint32_t)j, kk = NMZ_EDIT_DEL;
                        --i;
                    } else {
                        ka = (uint32_t)i, kb = (uint32_t)(j - 1), kk = NMZ_EDIT_INS;
                        --j;
                    }
                }
                if (kk != NMZ_NONE) {
                    if (tid == 0) s_ops[dist - 1 - found] = nmz_edit_op{ka, kb, kk};
                    ++found;
                }
            }
        }
        __syncthreads();
        if (tid == 0) g.dist[p] = dist;
        for (uint32_t s = tid; s < g.band; s += AW_THREADS) g.ops[p * g.band + s] = s_ops[s];
    }
}

}  // namespace nmz

struct nmz_ed_align_wide_plan {
    nmz_ctx *ctx = nullptr;
    uint32_t band = 0;
    uint64_t max_len = 0;
    uint32_t slots = 0;
    uint64_t slot_words = 0;
    nmz_ed_align_plan *narrow = nullptr;  // band <= NMZ_ALIGN_MAX_BAND: k_ed_align's plan does the work
    nmz::DevBuf hist;
    nmz::PlanFence fence;  // the slots serve one stream at a time (unused with a narrow plan, which has its own)
};

namespace nmz {

int aw_band(uint32_t band) {
    NMZ_CHECK(band <= NMZ_ALIGN_WIDE_MAX_BAND, "band " + std::to_string(band) +
                                                   " exceeds NMZ_ALIGN_WIDE_MAX_BAND (1024): edit scripts over wider "
                                                   "bands are not built yet");
    return NMZ_OK;
}

// every limit of nmz_ed_align_wide_pairs, no device; *max_len = the longest trace of the pairs
int aw_validate(const uint64_t *off, const uint64_t *sym, uint32_t n_traces, const uint32_t *pairs, uint64_t n_pairs,
                uint32_t band, const uint32_t *dist, const nmz_edit_op *ops, uint64_t *max_len) {
    return align_validate_for(aw_band, NMZ_ALIGN_WIDE_MAX_BAND, off, sym, n_traces, pairs, n_pairs, band, dist, ops,
                              max_len);
}

// the plan's shape for (band, max_len): no device. A band <= 64 has the narrow plan's shape.
int aw_shape(uint32_t band, uint64_t max_len, uint64_t *slot_words) {
    NMZ_TRY(aw_band(band));
    if (band <= NMZ_ALIGN_MAX_BAND) return align_shape(band, max_len, slot_words);
    NMZ_TRY(align_len("a trace of max_len", max_len));
    *slot_words = aw_blocks(max_len) * aw_block_words(aw_cells(band));
    return align_history_fits(max_len, *slot_words);
}

void aw_plan_destroy_locked(nmz_ed_align_wide_plan *p) {
    if (p->narrow) align_plan_destroy_locked(p->narrow);
    p->fence.destroy();
    p->hist.release();
    delete p;
}

int aw_plan_create_locked(nmz_ctx *ctx, uint32_t band, uint64_t max_len, uint64_t slot_words,
                          nmz_ed_align_wide_plan **out) {
    auto *p = new nmz_ed_align_wide_plan();
    p->ctx = ctx;
    p->band = band;
    p->max_len = max_len;
    p->slot_words = slot_words;
    int rc = NMZ_OK;
    if (band <= NMZ_ALIGN_MAX_BAND) {
        rc = align_plan_create_locked(ctx, band, max_len, slot_words, &p->narrow);
        if (rc == NMZ_OK) rc = nmz_ed_align_plan_info(p->narrow, &p->slots, nullptr);
    } else {
        p->slots = (uint32_t)std::max<uint64_t>(
            1, std::min<uint64_t>((uint64_t)std::max(ctx->n_cu, 1) * aw_slots_per_cu(aw_cells(band)),
                                  ALIGN_BUDGET / (slot_words * 8)));
        p->hist.pool = &ctx->pool;
        rc = p->hist.ensure((size_t)p->slots * slot_words * 8);
        if (rc == NMZ_OK) rc = p->fence.create("align wide plan");
    }
    if (rc != NMZ_OK) {
        aw_plan_destroy_locked(p);
        return rc;
    }
    *out = p;
    return NMZ_OK;
}

int aw_enqueue(nmz_ed_align_wide_plan *p, hipStream_t st, const uint64_t *d_off, const uint64_t *d_sym,
               const uint32_t *d_pairs, uint64_t n_pairs, uint32_t *d_dist, nmz_edit_op *d_ops) {
    if (p->narrow) return align_enqueue(p->narrow, st, d_off, d_sym, d_pairs, n_pairs, d_dist, d_ops);
    NMZ_CHECK(n_pairs <= (SIZE_MAX / sizeof(nmz_edit_op)) / NMZ_ALIGN_WIDE_MAX_BAND,
              "n_pairs * band does not fit the output");
    if (n_pairs == 0) return NMZ_OK;
    NMZ_CHECK(d_off && d_pairs && d_dist && d_ops, "d_off, d_pairs, d_dist or d_ops is NULL");
    NMZ_TRY(p->fence.enter(st));
    AwArgs a{d_off, d_sym, d_pairs, n_pairs, p->band, p->max_len, d_dist, d_ops, p->hist.as<uint64_t>(), p->slot_words};
    const unsigned blocks = (unsigned)std::min<uint64_t>(n_pairs, p->slots);
    int rc = NMZ_OK;
    {
        KernelTimer kt(p->ctx, st, "ed_align_wide");
        switch (aw_cells(p->band)) {
            case 1: hipLaunchKernelGGL(k_ed_align_wide<1>, dim3(blocks), dim3(AW_THREADS), 0, st, a); break;
            case 2: hipLaunchKernelGGL(k_ed_align_wide<2>, dim3(blocks), dim3(AW_THREADS), 0, st, a); break;
            case 3: hipLaunchKernelGGL(k_ed_align_wide<3>, dim3(blocks), dim3(AW_THREADS), 0, st, a); break;
            case 5: hipLaunchKernelGGL(k_ed_align_wide<5>, dim3(blocks), dim3(AW_THREADS), 0, st, a); break;
            default: hipLaunchKernelGGL(k_ed_align_wide<9>, dim3(blocks), dim3(AW_THREADS), 0, st, a); break;
        }
        if (hipGetLastError() != hipSuccess) rc = fail(NMZ_EHIP, "k_ed_align_wide launch failed");
    }
    NMZ_TRY(p->fence.leave(st));
    return rc;
}

// the host-arrays form behind nmz_ed_align_pairs and nmz_ed_align_wide_pairs, after their validation and shape
int align_pairs_call(nmz_ctx *ctx, const uint64_t *off, const uint64_t *sym, uint32_t n_traces, const uint32_t *pairs,
                     uint64_t n_pairs, uint32_t band, uint64_t max_len, uint64_t slot_words, uint32_t *dist,
                     nmz_edit_op *ops) {
    NMZ_CHECK(ctx != nullptr, "ctx is NULL");
    CtxGuard g(ctx);
    NMZ_TRY(g.rc);
    HostCall call(ctx);
    nmz_ed_align_wide_plan *plan = nullptr;
    NMZ_TRY(aw_plan_create_locked(ctx, band, max_len, slot_words, &plan));
    call.own_plan<aw_plan_destroy_locked>(plan);
    hipStream_t st = ctx->stream;
    const uint64_t total = off[n_traces];
    const size_t n_ops = (size_t)n_pairs * band;
    uint64_t *d_off, *d_sym;
    uint32_t *d_pairs, *d_dist;
    nmz_edit_op *d_ops;
    ScratchLayout lay;
    lay.add(&d_off, n_traces + 1).add(&d_sym, total + 1).add(&d_pairs, 2 * n_pairs).add(&d_dist, n_pairs);
    lay.add(&d_ops, n_ops + 1);
    NMZ_TRY(lay.bind(call.work));
    NMZ_TRY(upload_csr(d_off, d_sym, off, sym, n_traces, st));
    NMZ_TRY(copy_h2d(d_pairs, pairs, 2 * n_pairs, st));
    NMZ_TRY(aw_enqueue(plan, st, d_off, d_sym, d_pairs, n_pairs, d_dist, d_ops));
    NMZ_TRY(copy_d2h(dist, d_dist, n_pairs, st));
    NMZ_TRY(copy_d2h(ops, d_ops, n_ops, st));
    return call.done();
}

}  // namespace nmz

using namespace nmz;

extern "C" {

// One pair on the calling thread: the host aligner of ed_align.hip (align_host) with 16-bit cells, which hold
// band + 1 <= 1,025.
int nmz_ed_align_wide_host(const uint64_t *a, uint64_t n, const uint64_t *b, uint64_t m, uint32_t band, uint32_t *dist,
                           nmz_edit_op *ops) {
    NMZ_TRY(aw_band(band));
    return align_host<uint16_t>("nmz_ed_align_wide_host", "16-bit cells", a, n, b, m, band, dist, ops);
}

int nmz_ed_align_wide_plan_create(nmz_ctx *ctx, uint32_t band, uint64_t max_len, nmz_ed_align_wide_plan **out) {
    NMZ_CHECK(out != nullptr, "out is NULL");
    *out = nullptr;
    uint64_t slot_words = 0;
    NMZ_TRY(aw_shape(band, max_len, &slot_words));
    NMZ_CHECK(ctx != nullptr, "ctx is NULL");
    CtxGuard g(ctx);
    NMZ_TRY(g.rc);
    return aw_plan_create_locked(ctx, band, max_len, slot_words, out);
}

int nmz_ed_align_wide_plan_destroy(nmz_ed_align_wide_plan *plan) {
    if (!plan) return NMZ_OK;
    CtxGuard g(plan->ctx);
    NMZ_TRY(g.rc);
    aw_plan_destroy_locked(plan);
    return NMZ_OK;
}

int nmz_ed_align_wide_plan_info(const nmz_ed_align_wide_plan *plan, uint32_t *slots, uint64_t *history_bytes) {
    NMZ_CHECK(plan != nullptr, "plan is NULL");
    if (plan->narrow) return nmz_ed_align_plan_info(plan->narrow, slots, history_bytes);
    if (slots) *slots = plan->slots;
    if (history_bytes) *history_bytes = (uint64_t)plan->slots * plan->slot_words * 8;
    return NMZ_OK;
}

int nmz_ed_align_wide_pairs_dev(nmz_ed_align_wide_plan *plan, const uint64_t *d_off, const uint64_t *d_sym,
                                const uint32_t *d_pairs, uint64_t n_pairs, uint32_t *d_dist, nmz_edit_op *d_ops,
                                void *stream) {
    NMZ_CHECK(plan != nullptr, "plan is NULL");
    CtxGuard g(plan->ctx);
    NMZ_TRY(g.rc);
    return aw_enqueue(plan, stream ? (hipStream_t)stream : plan->ctx->stream, d_off, d_sym, d_pairs, n_pairs, d_dist,
                      d_ops);
}

int nmz_ed_align_wide_pairs(nmz_ctx *ctx, const uint64_t *off, const uint64_t *sym, uint32_t n_traces,
                            const uint32_t *pairs, uint64_t n_pairs, uint32_t band, uint32_t *dist, nmz_edit_op *ops) {
    // the arguments first: they are checked without a device
    uint64_t max_len = 0, slot_words = 0;
    NMZ_TRY(aw_validate(off, sym, n_traces, pairs, n_pairs, band, dist, ops, &max_len));
    if (n_pairs == 0) return NMZ_OK;  // nothing to write: no device either
    NMZ_TRY(aw_shape(band, max_len, &slot_words));
    return align_pairs_call(ctx, off, sym, n_traces, pairs, n_pairs, band, max_len, slot_words, dist, ops);
}

}  // extern "C"
