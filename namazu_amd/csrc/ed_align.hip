// K8 -- edit scripts for trace pairs: where two stored runs differ, not only how far apart they are
// (historystorage/historystorage.go:50-51 is the search interface this extends, naive/naive.go:235-257 the
// reference's equality search, util/trace/trace.go:29-31 SingleTrace.Equals: an empty script <=> Equals).
//
// For a pair (a, b) of n and m symbols and a band w <= 64: dist = ED_w(a, b) = min(Lev(a, b), w + 1), nmz_ed_pairs'
// value, and for dist <= w the canonical optimal alignment ("Edit scripts"): from (n, m) back
// to (0, 0) over the unit-cost matrix D, at (i, j) the first of diagonal (match or SUB), up (DEL), left (INS) that
// explains D[i][j]; the ops in forward order, matches omitted, then sentinels up to `band` slots.
//
// k_ed_align<C>: one wave per pair, grid-striding over the pairs; the workgroup is the
// wave and owns one history slot of the plan. The band's 2w + 1 cells of a row (cell d <-> j = i + d - w) lie
// blocked over the lanes, C in {1, 2, 3} consecutive cells per lane (w <= 31, <= 63, 64), so "up" (cell d + 1 of
// the previous row) is the lane's own next cell or one lane shift. The row step's arithmetic is ed_align_dev.h's,
// which K8w and K11 use too; this kernel's own are the lane shift for "up", the wave scan as the whole carry-in,
// where the ballots go, the history's layout and the walk. Per row:
//   1. t[d] = min(prev[d] + (a[i-1] != b[j-1]), prev[d + 1] + 1); a and the row block's window of b are staged in
//      LDS by coalesced loads once per 64 rows;
//   2. the horizontal closure D[d] = d + prefixmin(t[d'] - d'): a serial pass over the lane's cells, one 6-step
//      wave scan of the lanes' minima (DPP row shifts and broadcasts, no LDS);
//   3. two ballots per cell column c -- "diagonal accepted" and "diagonal ? symbols differ : up accepted" -- the
//      2 bits per band cell that name the walk's move at the cell. Lane r of the wave keeps row r's words of the
//      current 64-row block; one coalesced store per block writes them to the slot ([block][word][lane]);
//   4. the cut-off: no cell <= w ends the pair at dist = w + 1 before anything is walked.
// The walk reads the history a 64-row block at a time (coalesced, into LDS), newest block first, and steps through
// it with LDS reads only; dist is known, so the t-th op found goes to lane dist - 1 - t and the lanes store the
// pair's `band` slots in one pass. No scratch, no atomics; nothing is allocated per launch.
//
// Also here, for ed_align_wide.hip as well (nmz_internal.h): the host aligner align_host<Cell>, the validator body
// align_validate_for, and the length and budget checks.
#include <algorithm>
#include <new>
#include <string>
#include <vector>

#include "ed_align_dev.h"
#include "nmz_common.h"
#include "nmz_internal.h"

namespace nmz {

constexpr uint64_t ALIGN_MAX_LEN = 0xFFFFFFFFull;  // trace lengths 0 .. 2^32 - 2
constexpr uint32_t AL_SLOTS_PER_CU = 16;           // 4 waves per SIMD
static_assert(NMZ_ALIGN_MAX_BAND == 64, "a pair's ops fit one wave: one slot per lane");

struct AlArgs {
    const uint64_t *off, *sym;
    const uint32_t *pairs;
    uint64_t n_pairs;
    uint32_t band;
    uint64_t max_len;
    uint32_t *dist;
    nmz_edit_op *ops;
    uint64_t *hist;       // [slots][slot_words]
    uint64_t slot_words;  // blocks * 2 C * 64
};

template <int C>
__global__ __launch_bounds__(64) void k_ed_align(const AlArgs g) {
    __shared__ uint64_t s_a[ALIGN_ROWS];
    __shared__ uint64_t s_b[ALIGN_ROWS + 2 * NMZ_ALIGN_MAX_BAND];
    __shared__ uint64_t s_h[2 * C * ALIGN_ROWS];
    const uint32_t lane = threadIdx.x;
    const int32_t w = (int32_t)g.band, W2 = 2 * w;
    uint64_t *hist = g.hist + (uint64_t)blockIdx.x * g.slot_words;

    for (uint64_t p = blockIdx.x; p < g.n_pairs; p += gridDim.x) {
        const uint32_t ia = g.pairs[2 * p], ib = g.pairs[2 * p + 1];
        const uint64_t alo = g.off[ia], ahi = g.off[ia + 1], blo = g.off[ib], bhi = g.off[ib + 1];
        const uint64_t n64 = ahi > alo ? ahi - alo : 0, m64 = bhi > blo ? bhi - blo : 0;
        const uint64_t *__restrict__ a = g.sym + alo;
        const uint64_t *__restrict__ b = g.sym + blo;
        uint32_t dist;
        uint32_t op_a = NMZ_NONE, op_b = NMZ_NONE, op_k = NMZ_NONE;  // this lane's slot of the script

        if (n64 > g.max_len || m64 > g.max_len) {
            dist = NMZ_NONE;
        } else if ((n64 > m64 ? n64 - m64 : m64 - n64) > (uint64_t)w) {
            dist = (uint32_t)w + 1;  // the length filter
        } else {
            const int64_t n = (int64_t)n64, m = (int64_t)m64;
            // ---- forward: row 0, then the rows in blocks of 64
            int32_t prev[C];
            align_row0<C>(prev, (int32_t)lane * C, w, m);
            bool alive = true;
            for (int64_t i0 = 0; i0 < n && alive; i0 += ALIGN_ROWS) {
                const int32_t rows = (int32_t)min((int64_t)ALIGN_ROWS, n - i0);
                align_stage<int, 64>(s_a, s_b, a, n, b, m, i0, w, lane);
                uint64_t h1[C], h0[C];
#pragma unroll
                for (int c = 0; c < C; ++c) h1[c] = h0[c] = 0;
                for (int32_t r = 1; r <= rows; ++r) {
                    const int64_t i = i0 + r;
                    const uint64_t ai = s_a[r - 1];
                    const int32_t nxt = align_dpp<DPP_WAVE_SHL1>(ALIGN_INF, prev[0]);  // the next lane's first cell
                    int32_t t[C], lp[C];
                    bool valid[C];
                    AlignMoves<C> mv;
                    align_row_candidates<C>(prev, nxt, ai, s_b, r, (int32_t)lane * C, w, m, i, t, valid, lp, mv);
                    const int32_t excl = align_dpp<DPP_WAVE_SHR1>(ALIGN_INF, align_scan_min(lp[C - 1]));  // lanes below
                    const bool live = align_row_close<C>(prev, valid, lp, excl, (int32_t)lane * C, w, mv);
#pragma unroll
                    for (int c = 0; c < C; ++c) {  // lane r - 1 keeps row r's words
                        const uint64_t b1 = __ballot(mv.diag[c]), b0 = __ballot(mv.low[c]);
                        if ((int32_t)lane == r - 1) {
                            h1[c] = b1;
                            h0[c] = b0;
                        }
                    }
                    if (__ballot(live) == 0) {  // the band's minimum has passed w
                        alive = false;
                        break;
                    }
                }
                if (alive) {
                    uint64_t *hb = hist + (uint64_t)(i0 / ALIGN_ROWS) * (2 * C * 64);
#pragma unroll
                    for (int c = 0; c < C; ++c) {
                        hb[c * 64 + lane] = h1[c];
                        hb[(C + c) * 64 + lane] = h0[c];
                    }
                }
            }
            if (!alive) {
                dist = (uint32_t)w + 1;
            } else {
                const int32_t df = (int32_t)(m - n) + w;  // in [0, 2 w] behind the length filter
                dist = (uint32_t)min(__shfl(align_final_cell<C>(prev, df), df / C), w + 1);
            }
            // ---- the walk: every lane takes the same steps; lane dist - 1 - t keeps the t-th op found. The step is
            // written out here and in K8w, not shared: as a shared piece it cost this kernel 1.2 % at short traces
            // ("The aligners' shared pieces")
            if (dist >= 1 && dist <= (uint32_t)w) {
                __syncthreads();  // the history stores above, before the loads below
                int64_t i = n, j = m, loaded = -1;
                uint32_t found = 0;
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
                            const uint64_t *hb = hist + (uint64_t)blk * (2 * C * 64);
#pragma unroll
                            for (int k = 0; k < 2 * C; ++k) s_h[k * 64 + lane] = hb[k * 64 + lane];
                            __syncthreads();
                            loaded = blk;
                        }
                        const int64_t d = j - i + w;
                        if (d < 0 || d > W2) break;  // cannot happen on an optimal path of cost <= w
                        const uint32_t r = (uint32_t)((i - 1) % ALIGN_ROWS), c = (uint32_t)d % C, bit = (uint32_t)d / C;
                        const uint32_t m1 = (uint32_t)(s_h[c * 64 + r] >> bit) & 1u;
                        const uint32_t m0 = (uint32_t)(s_h[(C + c) * 64 + r] >> bit) & 1u;
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
                        if (lane == dist - 1 - found) op_a = ka, op_b = kb, op_k = kk;
                        ++found;
                    }
                }
            }
        }
        if (lane == 0) g.dist[p] = dist;
        if (lane < g.band) {
            nmz_edit_op *__restrict__ o = g.ops + p * g.band + lane;
            o->a_pos = op_a;
            o->b_pos = op_b;
            o->kind = op_k;
        }
    }
}

}  // namespace nmz

struct nmz_ed_align_plan {
    nmz_ctx *ctx = nullptr;
    uint32_t band = 0;
    uint64_t max_len = 0;
    uint32_t slots = 0;
    uint64_t slot_words = 0;
    nmz::DevBuf hist;
    nmz::PlanFence fence;  // the slots serve one stream at a time
};

namespace nmz {

int align_band(uint32_t band) {
    NMZ_CHECK(band <= NMZ_ALIGN_MAX_BAND, "band " + std::to_string(band) +
                                              " exceeds NMZ_ALIGN_MAX_BAND (64): edit scripts over wider bands are "
                                              "not built yet");
    return NMZ_OK;
}

int align_len(const std::string &what, uint64_t len) {
    NMZ_CHECK(len < ALIGN_MAX_LEN, what + " has " + std::to_string(len) + " elements: at most 2^32 - 2");
    return NMZ_OK;
}

int align_history_fits(uint64_t max_len, uint64_t slot_words) {
    NMZ_CHECK(slot_words * 8 <= ALIGN_BUDGET,
              "max_len " + std::to_string(max_len) + ": one pair's history (" + std::to_string(slot_words * 8) +
                  " bytes) exceeds the plan's budget of " + std::to_string(ALIGN_BUDGET) + " bytes");
    return NMZ_OK;
}

int align_validate_for(int (*band_ok)(uint32_t), uint32_t max_band, const uint64_t *off, const uint64_t *sym,
                       uint32_t n_traces, const uint32_t *pairs, uint64_t n_pairs, uint32_t band, const uint32_t *dist,
                       const nmz_edit_op *ops, uint64_t *max_len) {
    NMZ_TRY(band_ok(band));
    *max_len = 0;
    if (n_pairs == 0) return NMZ_OK;
    NMZ_CHECK(n_pairs <= (SIZE_MAX / sizeof(nmz_edit_op)) / max_band, "n_pairs * band does not fit the output");
    NMZ_CHECK(off && pairs && dist, "off, pairs or dist is NULL");
    NMZ_CHECK(band == 0 || ops, "ops is NULL");
    for (uint64_t t = 0; t < 2 * n_pairs; ++t)
        NMZ_CHECK(pairs[t] < n_traces, "pair index out of range (pair " + std::to_string(t / 2) + ")");
    for (uint32_t t = 0; t < n_traces; ++t) {
        NMZ_CHECK(off[t] <= off[t + 1], "offsets must be non-decreasing (trace " + std::to_string(t) + ")");
        NMZ_TRY(align_len("trace " + std::to_string(t), off[t + 1] - off[t]));
    }
    for (uint64_t t = 0; t < 2 * n_pairs; ++t) *max_len = std::max(*max_len, off[pairs[t] + 1] - off[pairs[t]]);
    NMZ_CHECK(off[n_traces] == off[0] || sym, "sym is NULL");
    return NMZ_OK;
}

// every limit of nmz_ed_align_pairs, no device; *max_len = the longest trace of the pairs
int align_validate(const uint64_t *off, const uint64_t *sym, uint32_t n_traces, const uint32_t *pairs,
                   uint64_t n_pairs, uint32_t band, const uint32_t *dist, const nmz_edit_op *ops, uint64_t *max_len) {
    return align_validate_for(align_band, NMZ_ALIGN_MAX_BAND, off, sym, n_traces, pairs, n_pairs, band, dist, ops,
                              max_len);
}

// the plan's shape for (band, max_len): no device
int align_shape(uint32_t band, uint64_t max_len, uint64_t *slot_words) {
    NMZ_TRY(align_band(band));
    NMZ_TRY(align_len("a trace of max_len", max_len));
    *slot_words = std::max<uint64_t>(1, (max_len + ALIGN_ROWS - 1) / ALIGN_ROWS) * 2 * align_cells(band) * 64;
    return align_history_fits(max_len, *slot_words);
}

void align_plan_destroy_locked(nmz_ed_align_plan *p) {
    p->fence.destroy();
    p->hist.release();
    delete p;
}

int align_plan_create_locked(nmz_ctx *ctx, uint32_t band, uint64_t max_len, uint64_t slot_words,
                             nmz_ed_align_plan **out) {
    auto *p = new nmz_ed_align_plan();
    p->ctx = ctx;
    p->band = band;
    p->max_len = max_len;
    p->slot_words = slot_words;
    p->slots = (uint32_t)std::max<uint64_t>(
        1, std::min<uint64_t>((uint64_t)std::max(ctx->n_cu, 1) * AL_SLOTS_PER_CU, ALIGN_BUDGET / (slot_words * 8)));
    p->hist.pool = &ctx->pool;
    int rc = p->hist.ensure((size_t)p->slots * slot_words * 8);
    if (rc == NMZ_OK) rc = p->fence.create("align plan");
    if (rc != NMZ_OK) {
        align_plan_destroy_locked(p);
        return rc;
    }
    *out = p;
    return NMZ_OK;
}

int align_enqueue(nmz_ed_align_plan *p, hipStream_t st, const uint64_t *d_off, const uint64_t *d_sym,
                  const uint32_t *d_pairs, uint64_t n_pairs, uint32_t *d_dist, nmz_edit_op *d_ops) {
    NMZ_CHECK(n_pairs <= (SIZE_MAX / sizeof(nmz_edit_op)) / NMZ_ALIGN_MAX_BAND,
              "n_pairs * band does not fit the output");
    if (n_pairs == 0) return NMZ_OK;
    NMZ_CHECK(d_off && d_pairs && d_dist, "d_off, d_pairs or d_dist is NULL");
    NMZ_CHECK(p->band == 0 || d_ops, "d_ops is NULL");
    NMZ_TRY(p->fence.enter(st));
    AlArgs a{d_off, d_sym, d_pairs, n_pairs, p->band, p->max_len, d_dist, d_ops, p->hist.as<uint64_t>(), p->slot_words};
    const unsigned blocks = (unsigned)std::min<uint64_t>(n_pairs, p->slots);
    int rc = NMZ_OK;
    {
        KernelTimer kt(p->ctx, st, "ed_align");
        switch (align_cells(p->band)) {
            case 1: hipLaunchKernelGGL(k_ed_align<1>, dim3(blocks), dim3(64), 0, st, a); break;
            case 2: hipLaunchKernelGGL(k_ed_align<2>, dim3(blocks), dim3(64), 0, st, a); break;
            default: hipLaunchKernelGGL(k_ed_align<3>, dim3(blocks), dim3(64), 0, st, a); break;
        }
        if (hipGetLastError() != hipSuccess) rc = fail(NMZ_EHIP, "k_ed_align launch failed");
    }
    NMZ_TRY(p->fence.leave(st));
    return rc;
}

// One pair on the calling thread (historystorage.go:50-51, naive.go:235-257, util/trace/trace.go:29-31): the
// +inf-banded matrix kept whole, row by row, in cells of type Cell (values capped at w + 1, which leaves every value
// <= w exact), then the walk by the definition. No ballots, no closure scan, no packed history: nothing shared with
// the kernels.
template <typename Cell>
int align_host(const char *fn, const char *cells, const uint64_t *a, uint64_t n, const uint64_t *b, uint64_t m,
               uint32_t band, uint32_t *dist, nmz_edit_op *ops) {
    NMZ_TRY(align_len("a", n));
    NMZ_TRY(align_len("b", m));
    NMZ_CHECK((n == 0 || a) && (m == 0 || b), "a or b is NULL");
    NMZ_CHECK(dist != nullptr, "dist is NULL");
    NMZ_CHECK(band == 0 || ops, "ops is NULL");
    for (uint32_t s = 0; s < band; ++s) ops[s] = nmz_edit_op{NMZ_NONE, NMZ_NONE, NMZ_NONE};
    const int64_t w = band, W = 2 * w + 1, N = (int64_t)n, M = (int64_t)m;
    const Cell cap = (Cell)(band + 1);
    if ((n > m ? n - m : m - n) > band) {
        *dist = band + 1;
        return NMZ_OK;
    }
    std::vector<Cell> D;
    try {
        D.assign((size_t)(N + 1) * (size_t)W, cap);  // D[i][k]: the cell (i, j = i + k - w)
    } catch (const std::exception &) {  // bad_alloc; (n + 1) * W < 2^44 cells is far below max_size(): no length_error
        return fail(NMZ_ENOMEM, std::string(fn) + ": the band rows of " + std::to_string(n) + " x " +
                                    std::to_string(W) + " " + cells + " do not fit the host's memory");
    }
    auto at = [&](int64_t i, int64_t k) -> Cell & { return D[(size_t)i * (size_t)W + (size_t)k]; };
    for (int64_t j = 0; j <= std::min(M, w); ++j) at(0, j + w) = (Cell)j;
    for (int64_t i = 1; i <= N; ++i)
        for (int64_t k = 0; k < W; ++k) {
            const int64_t j = i + k - w;
            if (j < 0 || j > M) continue;
            int64_t v = cap;
            if (j >= 1) v = std::min<int64_t>(v, at(i - 1, k) + (a[i - 1] != b[j - 1] ? 1 : 0));
            if (k + 1 < W) v = std::min<int64_t>(v, at(i - 1, k + 1) + 1);
            if (k >= 1 && j >= 1) v = std::min<int64_t>(v, at(i, k - 1) + 1);
            at(i, k) = (Cell)v;
        }
    const uint32_t d = at(N, M - N + w);
    *dist = d;
    if (d > band) return NMZ_OK;
    int64_t i = N, j = M;
    uint32_t found = 0;
    while ((i > 0 || j > 0) && found < d) {
        const int64_t k = j - i + w;
        const int64_t cur = at(i, k);
        nmz_edit_op op{NMZ_NONE, NMZ_NONE, NMZ_NONE};
        if (i > 0 && j > 0 && at(i - 1, k) + (a[i - 1] != b[j - 1] ? 1 : 0) == cur) {
            if (a[i - 1] != b[j - 1]) op = nmz_edit_op{(uint32_t)(i - 1), (uint32_t)(j - 1), NMZ_EDIT_SUB};
            --i, --j;
        } else if (i > 0 && k + 1 < W && at(i - 1, k + 1) + 1 == cur) {
            op = nmz_edit_op{(uint32_t)(i - 1), (uint32_t)j, NMZ_EDIT_DEL};
            --i;
        } else {
            if (j == 0) return fail(NMZ_EINVAL, std::string(fn) + ": the walk left the matrix");  // not reachable
            op = nmz_edit_op{(uint32_t)i, (uint32_t)(j - 1), NMZ_EDIT_INS};
            --j;
        }
        if (op.kind != NMZ_NONE) ops[d - 1 - found++] = op;
    }
    return NMZ_OK;
}
template int align_host<uint8_t>(const char *, const char *, const uint64_t *, uint64_t, const uint64_t *, uint64_t,
                                 uint32_t, uint32_t *, nmz_edit_op *);
template int align_host<uint16_t>(const char *, const char *, const uint64_t *, uint64_t, const uint64_t *, uint64_t,
                                  uint32_t, uint32_t *, nmz_edit_op *);

}  // namespace nmz

using namespace nmz;

extern "C" {

int nmz_ed_align_host(const uint64_t *a, uint64_t n, const uint64_t *b, uint64_t m, uint32_t band, uint32_t *dist,
                      nmz_edit_op *ops) {
    NMZ_TRY(align_band(band));
    return align_host<uint8_t>("nmz_ed_align_host", "cells", a, n, b, m, band, dist, ops);
}

int nmz_ed_align_plan_create(nmz_ctx *ctx, uint32_t band, uint64_t max_len, nmz_ed_align_plan **out) {
    NMZ_CHECK(out != nullptr, "out is NULL");
    *out = nullptr;
    uint64_t slot_words = 0;
    NMZ_TRY(align_shape(band, max_len, &slot_words));
    NMZ_CHECK(ctx != nullptr, "ctx is NULL");
    CtxGuard g(ctx);
    NMZ_TRY(g.rc);
    return align_plan_create_locked(ctx, band, max_len, slot_words, out);
}

int nmz_ed_align_plan_destroy(nmz_ed_align_plan *plan) {
    if (!plan) return NMZ_OK;
    CtxGuard g(plan->ctx);
    NMZ_TRY(g.rc);
    align_plan_destroy_locked(plan);
    return NMZ_OK;
}

int nmz_ed_align_plan_info(const nmz_ed_align_plan *plan, uint32_t *slots, uint64_t *history_bytes) {
    NMZ_CHECK(plan != nullptr, "plan is NULL");
    if (slots) *slots = plan->slots;
    if (history_bytes) *history_bytes = (uint64_t)plan->slots * plan->slot_words * 8;
    return NMZ_OK;
}

int nmz_ed_align_pairs_dev(nmz_ed_align_plan *plan, const uint64_t *d_off, const uint64_t *d_sym,
                           const uint32_t *d_pairs, uint64_t n_pairs, uint32_t *d_dist, nmz_edit_op *d_ops,
                           void *stream) {
    NMZ_CHECK(plan != nullptr, "plan is NULL");
    CtxGuard g(plan->ctx);
    NMZ_TRY(g.rc);
    return align_enqueue(plan, stream ? (hipStream_t)stream : plan->ctx->stream, d_off, d_sym, d_pairs, n_pairs, d_dist,
                         d_ops);
}

int nmz_ed_align_pairs(nmz_ctx *ctx, const uint64_t *off, const uint64_t *sym, uint32_t n_traces, const uint32_t *pairs,
                       uint64_t n_pairs, uint32_t band, uint32_t *dist, nmz_edit_op *ops) {
    // the arguments first: they are checked without a device
    uint64_t max_len = 0, slot_words = 0;
    NMZ_TRY(align_validate(off, sym, n_traces, pairs, n_pairs, band, dist, ops, &max_len));
    if (n_pairs == 0) return NMZ_OK;  // nothing to write: no device either
    NMZ_TRY(align_shape(band, max_len, &slot_words));
    return align_pairs_call(ctx, off, sym, n_traces, pairs, n_pairs, band, max_len, slot_words, dist, ops);
}

}  // extern "C"
