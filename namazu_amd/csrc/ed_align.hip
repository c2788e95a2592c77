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
// the previous row) is the lane's own next cell or one lane shift. Per row:
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
#include <algorithm>
#include <new>
#include <string>
#include <vector>

#include "nmz_common.h"
#include "nmz_internal.h"

namespace nmz {

constexpr uint32_t AL_ROWS = 64;                   // rows per staged block: one history row per lane
constexpr int32_t AL_INF = 1 << 28;                // beyond any value a live row holds (<= 3 w + 1)
constexpr uint64_t AL_MAX_LEN = 0xFFFFFFFFull;     // trace lengths 0 .. 2^32 - 2
constexpr size_t AL_BUDGET = (size_t)256 << 20;    // the plan's history scratch, all slots together
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

// cells per lane for a band
static int al_cells(uint32_t band) { return band <= 31 ? 1 : (band <= 63 ? 2 : 3); }
static uint64_t al_blocks(uint64_t max_len) { return std::max<uint64_t>(1, (max_len + AL_ROWS - 1) / AL_ROWS); }

// Cross-lane moves of the row step as DPP modifiers (data-parallel primitives: no LDS round trip, unlike __shfl).
// A lane without a source -- off the row's end, or in a row the mask leaves out -- keeps `old`.
constexpr int AL_ROW_SHR = 0x110, AL_ROW_BCAST15 = 0x142, AL_ROW_BCAST31 = 0x143;  // row_shr:n = AL_ROW_SHR + n
constexpr int AL_WAVE_SHL1 = 0x130, AL_WAVE_SHR1 = 0x138;                          // lane i takes lane i + 1 / i - 1
template <int CTRL, int ROW_MASK = 0xF>
__device__ __forceinline__ int32_t al_dpp(int32_t old, int32_t v) {
    return __builtin_amdgcn_update_dpp(old, v, CTRL, ROW_MASK, 0xF, false);
}
// inclusive minimum over lanes 0 .. lane: four steps inside each row of 16 lanes, then row 0's last lane into row 1
// and row 2's into row 3, then row 1's last lane into rows 2 and 3
__device__ __forceinline__ int32_t al_scan_min(int32_t v) {
    v = min(v, al_dpp<AL_ROW_SHR + 1>(AL_INF, v));
    v = min(v, al_dpp<AL_ROW_SHR + 2>(AL_INF, v));
    v = min(v, al_dpp<AL_ROW_SHR + 4>(AL_INF, v));
    v = min(v, al_dpp<AL_ROW_SHR + 8>(AL_INF, v));
    v = min(v, al_dpp<AL_ROW_BCAST15, 0xA>(AL_INF, v));
    v = min(v, al_dpp<AL_ROW_BCAST31, 0xC>(AL_INF, v));
    return v;
}

template <int C>
__global__ __launch_bounds__(64) void k_ed_align(const AlArgs g) {
    __shared__ uint64_t s_a[AL_ROWS];
    __shared__ uint64_t s_b[AL_ROWS + 2 * NMZ_ALIGN_MAX_BAND];
    __shared__ uint64_t s_h[2 * C * AL_ROWS];
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
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const int32_t d = (int32_t)lane * C + c;
                const int64_t jv = (int64_t)d - w;
                prev[c] = (d <= W2 && jv >= 0 && jv <= m) ? (int32_t)jv : AL_INF;
            }
            bool alive = true;
            for (int64_t i0 = 0; i0 < n && alive; i0 += AL_ROWS) {
                const int32_t rows = (int32_t)min((int64_t)AL_ROWS, n - i0);
                __syncthreads();  // the previous block's reads of s_a / s_b
                s_a[lane] = i0 + lane < n ? a[i0 + lane] : 0;
                for (int32_t t = (int32_t)lane; t < (int32_t)AL_ROWS + W2; t += 64) {
                    const int64_t jb = i0 - w + t;
                    s_b[t] = (jb >= 0 && jb < m) ? b[jb] : 0;
                }
                __syncthreads();
                uint64_t h1[C], h0[C];
#pragma unroll
                for (int c = 0; c < C; ++c) h1[c] = h0[c] = 0;
                for (int32_t r = 1; r <= rows; ++r) {
                    const int64_t i = i0 + r;
                    const uint64_t ai = s_a[r - 1];
                    const int32_t nxt = al_dpp<AL_WAVE_SHL1>(AL_INF, prev[0]);  // cell d + 1 of the lane's last cell
                    int32_t t[C], dg[C], up[C];
                    bool valid[C], ne[C];
#pragma unroll
                    for (int c = 0; c < C; ++c) {
                        const int32_t d = (int32_t)lane * C + c;
                        const int64_t jv = i + d - w;
                        valid[c] = d <= W2 && jv >= 0 && jv <= m;
                        const uint64_t bj = s_b[valid[c] ? r + d - 1 : 0];  // b[jv - 1]
                        ne[c] = ai != bj;
                        dg[c] = jv >= 1 ? prev[c] + (ne[c] ? 1 : 0) : AL_INF;
                        up[c] = (c + 1 < C ? prev[c + 1 < C ? c + 1 : c] : nxt) + 1;
                        t[c] = valid[c] ? min(dg[c], up[c]) : AL_INF;
                    }
                    // D[d] = d + min over d' <= d of (t[d'] - d')
                    int32_t lp[C];
                    lp[0] = t[0] - (int32_t)lane * C;
#pragma unroll
                    for (int c = 1; c < C; ++c) lp[c] = min(lp[c - 1], t[c] - ((int32_t)lane * C + c));
                    const int32_t excl = al_dpp<AL_WAVE_SHR1>(AL_INF, al_scan_min(lp[C - 1]));  // lanes below this one
                    bool live = false;
#pragma unroll
                    for (int c = 0; c < C; ++c) {
                        const int32_t d = (int32_t)lane * C + c;
                        const int32_t cur = valid[c] ? min(d + min(excl, lp[c]), AL_INF) : AL_INF;
                        const bool diag = valid[c] && dg[c] == cur && cur < AL_INF;
                        const bool low = diag ? ne[c] : (valid[c] && up[c] == cur && cur < AL_INF);
                        const uint64_t b1 = __ballot(diag), b0 = __ballot(low);
                        if ((int32_t)lane == r - 1) {
                            h1[c] = b1;
                            h0[c] = b0;
                        }
                        live = live || cur <= w;
                        prev[c] = cur;
                    }
                    if (__ballot(live) == 0) {  // the band's minimum has passed w
                        alive = false;
                        break;
                    }
                }
                if (alive) {
                    uint64_t *hb = hist + (uint64_t)(i0 / AL_ROWS) * (2 * C * 64);
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
                int32_t v = prev[0];
#pragma unroll
                for (int c = 1; c < C; ++c) v = (df % C) == c ? prev[c] : v;
                v = __shfl(v, df / C);
                dist = (uint32_t)min(v, w + 1);
            }
            // ---- the walk: every lane takes the same steps; lane dist - 1 - t keeps the t-th op found
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
                        const int64_t blk = (i - 1) / AL_ROWS;
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
                        const uint32_t r = (uint32_t)((i - 1) % AL_ROWS), c = (uint32_t)d % C, bit = (uint32_t)d / C;
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
    // the stream the plan's launches were enqueued on last, with an event after the latest one (destroy waits)
    hipStream_t last = nullptr;
    hipEvent_t ev = nullptr;
};

namespace nmz {

int align_band(uint32_t band) {
    NMZ_CHECK(band <= NMZ_ALIGN_MAX_BAND, "band " + std::to_string(band) +
                                              " exceeds NMZ_ALIGN_MAX_BAND (64): edit scripts over wider bands are "
                                              "not built yet");
    return NMZ_OK;
}

static int align_len(const std::string &what, uint64_t len) {
    NMZ_CHECK(len < AL_MAX_LEN, what + " has " + std::to_string(len) + " elements: at most 2^32 - 2");
    return NMZ_OK;
}

// every limit of nmz_ed_align_pairs, no device; *max_len = the longest trace of the pairs
int align_validate(const uint64_t *off, const uint64_t *sym, uint32_t n_traces, const uint32_t *pairs,
                   uint64_t n_pairs, uint32_t band, const uint32_t *dist, const nmz_edit_op *ops, uint64_t *max_len) {
    NMZ_TRY(align_band(band));
    *max_len = 0;
    if (n_pairs == 0) return NMZ_OK;
    NMZ_CHECK(n_pairs <= (SIZE_MAX / sizeof(nmz_edit_op)) / NMZ_ALIGN_MAX_BAND,
              "n_pairs * band does not fit the output");
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

// the plan's shape for (band, max_len): no device
int align_shape(uint32_t band, uint64_t max_len, uint64_t *slot_words) {
    NMZ_TRY(align_band(band));
    NMZ_TRY(align_len("a trace of max_len", max_len));
    *slot_words = al_blocks(max_len) * 2 * al_cells(band) * 64;
    NMZ_CHECK(*slot_words * 8 <= AL_BUDGET,
              "max_len " + std::to_string(max_len) + ": one pair's history (" + std::to_string(*slot_words * 8) +
                  " bytes) exceeds the plan's budget of " + std::to_string(AL_BUDGET) + " bytes");
    return NMZ_OK;
}

void align_plan_destroy_locked(nmz_ed_align_plan *p) {
    if (p->ev) {
        (void)hipEventSynchronize(p->ev);
        (void)hipEventDestroy(p->ev);
    }
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
        1, std::min<uint64_t>((uint64_t)std::max(ctx->n_cu, 1) * AL_SLOTS_PER_CU, AL_BUDGET / (slot_words * 8)));
    p->hist.pool = &ctx->pool;
    int rc = p->hist.ensure((size_t)p->slots * slot_words * 8);
    if (rc == NMZ_OK && hipEventCreateWithFlags(&p->ev, hipEventDisableTiming) != hipSuccess)
        rc = fail(NMZ_EHIP, "align plan: hipEventCreate failed");
    if (rc != NMZ_OK) {
        p->ev = nullptr;
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
    if (p->last && p->last != st) NMZ_HIP(hipStreamWaitEvent(st, p->ev, 0));  // the slots serve one stream at a time
    AlArgs a{d_off, d_sym, d_pairs, n_pairs, p->band, p->max_len, d_dist, d_ops, p->hist.as<uint64_t>(), p->slot_words};
    const unsigned blocks = (unsigned)std::min<uint64_t>(n_pairs, p->slots);
    int rc = NMZ_OK;
    {
        KernelTimer kt(p->ctx, st, "ed_align");
        switch (al_cells(p->band)) {
            case 1: hipLaunchKernelGGL(k_ed_align<1>, dim3(blocks), dim3(64), 0, st, a); break;
            case 2: hipLaunchKernelGGL(k_ed_align<2>, dim3(blocks), dim3(64), 0, st, a); break;
            default: hipLaunchKernelGGL(k_ed_align<3>, dim3(blocks), dim3(64), 0, st, a); break;
        }
        if (hipGetLastError() != hipSuccess) rc = fail(NMZ_EHIP, "k_ed_align launch failed");
    }
    p->last = st;
    NMZ_HIP(hipEventRecord(p->ev, st));
    return rc;
}

}  // namespace nmz

using namespace nmz;

extern "C" {

// One pair on the calling thread (historystorage.go:50-51, naive.go:235-257, util/trace/trace.go:29-31): the
// +inf-banded matrix kept whole, row by row (values capped at w + 1, which leaves every value <= w exact), then the
// walk by the definition. No ballots, no closure scan, no packed history: nothing shared with the kernel.
int nmz_ed_align_host(const uint64_t *a, uint64_t n, const uint64_t *b, uint64_t m, uint32_t band, uint32_t *dist,
                      nmz_edit_op *ops) {
    NMZ_TRY(align_band(band));
    NMZ_TRY(align_len("a", n));
    NMZ_TRY(align_len("b", m));
    NMZ_CHECK((n == 0 || a) && (m == 0 || b), "a or b is NULL");
    NMZ_CHECK(dist != nullptr, "dist is NULL");
    NMZ_CHECK(band == 0 || ops, "ops is NULL");
    for (uint32_t s = 0; s < band; ++s) ops[s] = nmz_edit_op{NMZ_NONE, NMZ_NONE, NMZ_NONE};
    const int64_t w = band, W = 2 * w + 1, N = (int64_t)n, M = (int64_t)m;
    const uint8_t cap = (uint8_t)(band + 1);
    if ((n > m ? n - m : m - n) > band) {
        *dist = band + 1;
        return NMZ_OK;
    }
    std::vector<uint8_t> D;
    try {
        D.assign((size_t)(N + 1) * (size_t)W, cap);  // D[i][k]: the cell (i, j = i + k - w)
    } catch (const std::bad_alloc &) {
        return fail(NMZ_ENOMEM, "nmz_ed_align_host: the band rows of " + std::to_string(n) + " x " + std::to_string(W) +
                                    " cells do not fit the host's memory");
    }
    auto at = [&](int64_t i, int64_t k) -> uint8_t & { return D[(size_t)i * (size_t)W + (size_t)k]; };
    for (int64_t j = 0; j <= std::min(M, w); ++j) at(0, j + w) = (uint8_t)j;
    for (int64_t i = 1; i <= N; ++i)
        for (int64_t k = 0; k < W; ++k) {
            const int64_t j = i + k - w;
            if (j < 0 || j > M) continue;
            int64_t v = cap;
            if (j >= 1) v = std::min<int64_t>(v, at(i - 1, k) + (a[i - 1] != b[j - 1] ? 1 : 0));
            if (k + 1 < W) v = std::min<int64_t>(v, at(i - 1, k + 1) + 1);
            if (k >= 1 && j >= 1) v = std::min<int64_t>(v, at(i, k - 1) + 1);
            at(i, k) = (uint8_t)v;
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
            if (j == 0) return fail(NMZ_EINVAL, "nmz_ed_align_host: the walk left the matrix");  // not reachable
            op = nmz_edit_op{(uint32_t)i, (uint32_t)(j - 1), NMZ_EDIT_INS};
            --j;
        }
        if (op.kind != NMZ_NONE) ops[d - 1 - found++] = op;
    }
    return NMZ_OK;
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
    NMZ_CHECK(ctx != nullptr, "ctx is NULL");
    CtxGuard g(ctx);
    NMZ_TRY(g.rc);
    HostCall call(ctx);
    nmz_ed_align_plan *plan = nullptr;
    NMZ_TRY(align_plan_create_locked(ctx, band, max_len, slot_words, &plan));
    call.own_plan<align_plan_destroy_locked>(plan);
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
    NMZ_TRY(align_enqueue(plan, st, d_off, d_sym, d_pairs, n_pairs, d_dist, d_ops));
    NMZ_TRY(copy_d2h(dist, d_dist, n_pairs, st));
    NMZ_TRY(copy_d2h(ops, d_ops, n_ops, st));
    return call.done();
}

}  // extern "C"
