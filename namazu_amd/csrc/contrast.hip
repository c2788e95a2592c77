// K6 -- order contrast: the event pairs whose order separates failing runs from passing ones
// (historystorage/naive/naive.go:199-213 IsSuccessful labels the runs; cli/tools/summary.go:40-57 lists them).
//
// For pos[R][E] (the position of event e in recorded run r, NMZ_NONE = absent) and failed[R], every ordered pair
// (b, a), b != a:
//     F(b,a) = #{failing r : both present, pos[r][b] < pos[r][a]}      P(b,a) = the same over passing runs
//     score  = F * n_pass - P * n_fail                                  (int64)
// ranked by (score desc, F desc, b * E + a asc); only score > 0 is listed (include/nmz_gpu.h).
//
// Kernels:
//   k_contrast_runs   one workgroup: a stable partition of the run indices, failing runs first (perm[R]), n_fail and
//                     n_pass into the info record, n_positive zeroed.
//   k_contrast_sweep  <FULL>: a workgroup owns 64 `a` columns x 32 `b` rows of the pair matrix, and its four waves
//                     deal the runs among themselves (wave w takes every fourth failing run and every fourth
//                     passing run). No LDS for the operands: a lane owns one `a` column and reads pos[r][a]
//                     coalesced (absent -> 0 on load, so nothing is less than it); the 32 `b` values of the run are
//                     wave-uniform scalar loads (absent stays NMZ_NONE, never less than anything), so one unsigned
//                     compare with an SGPR operand is the exact predicate and a carry-in add counts it. One counter
//                     register per b: the failing runs are counted first, the counters are shifted left by 16, the
//                     passing runs follow -- F << 16 | P (n_fail + n_pass <= 65,535, so neither half overflows,
//                     in a wave or in the sum). The waves add their counters into 8 KB of LDS; then wave w holds
//                     rows 8 w .. 8 w + 7, forms the scores, writes the optional counts (coalesced along a), and
//                     the tile's 2,048 pairs feed one block selection (topk_block_select<true>) with
//                     n_fault = 0, sum_delay_ns = score * 2^16 + F, seed = b * E + a, first_fault = P; the
//                     positive pairs go to n_positive with one atomic per workgroup.
//   topk_merge_lists  the per-workgroup lists (topk.hip).
//   k_contrast_pairs  one wave per winner: recounts the reverse direction (a, b) over the runs and writes the
//                     nmz_order_pair; sentinels past the positive pairs.
// Nothing of size E^2 is written or allocated unless the caller asks for the counts.
#include <algorithm>
#include <string>
#include <vector>

#include "nmz_common.h"
#include "nmz_internal.h"
#include "topk_dev.h"

namespace nmz {

constexpr uint32_t CT_MAX_EVENTS = NMZ_DELIVERY_MAX_EVENTS;
constexpr uint32_t CT_MAX_RUNS = NMZ_CONTRAST_MAX_RUNS;
constexpr uint32_t CT_COLS = 64;                 // `a` columns per workgroup, one per lane
constexpr uint32_t CT_WAVES = TOPK_THREADS / 64;  // the tile's runs are dealt over the waves
constexpr uint32_t CT_ROWS = 32;                 // `b` rows per workgroup: 32 compares per column load
static_assert(CT_COLS * CT_ROWS == TOPK_CHUNK, "a tile is one selection");
static_assert(CT_ROWS == CT_WAVES * TOPK_PER_THREAD, "wave w selects over rows 8 w .. 8 w + 7");
constexpr uint32_t CT_RUNS_THREADS = 1024;

static_assert(sizeof(nmz_order_pair) == 32, "nmz_order_pair layout");
static_assert(sizeof(nmz_pair_counts) == 8, "nmz_pair_counts layout");
static_assert(sizeof(nmz_contrast_info) == 16, "nmz_contrast_info layout");

// perm[0 .. n_fail) = the failing runs in index order, perm[n_fail .. R) = the passing ones; any nonzero label fails
__global__ __launch_bounds__(CT_RUNS_THREADS) void k_contrast_runs(const uint8_t *__restrict__ failed, uint32_t R,
                                                                    uint32_t *__restrict__ perm,
                                                                    nmz_contrast_info *__restrict__ info) {
    __shared__ uint32_t part[CT_RUNS_THREADS];
    const uint32_t t = threadIdx.x;
    const uint32_t chunk = (R + CT_RUNS_THREADS - 1) / CT_RUNS_THREADS;
    const uint32_t lo = min(t * chunk, R), hi = min(lo + chunk, R);
    uint32_t c = 0;
    for (uint32_t r = lo; r < hi; ++r) c += failed[r] ? 1u : 0u;
    part[t] = c;
    __syncthreads();
    for (uint32_t d = 1; d < CT_RUNS_THREADS; d <<= 1) {
        const uint32_t v = t >= d ? part[t - d] : 0u;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    const uint32_t total = part[CT_RUNS_THREADS - 1];
    uint32_t f = part[t] - c;           // failing runs before lo
    uint32_t p = total + (lo - f);      // passing runs before lo, behind every failing run
    for (uint32_t r = lo; r < hi; ++r) {
        if (failed[r])
            perm[f++] = r;
        else
            perm[p++] = r;
    }
    if (t == 0) {
        info->n_fail = total;
        info->n_pass = R - total;
        info->n_positive = 0;
    }
}

// this wave's runs perm[first], perm[first + CT_WAVES], ... (below end <= R) into
// cnt[j] += (pos[r][b0 + j] < pos[r][a]): v_cmp with the scalar b side, carry-in add
template <bool FULL>
__device__ __forceinline__ void ct_count(const uint32_t *__restrict__ pos, const uint32_t *__restrict__ perm,
                                         uint32_t first, uint32_t end, uint32_t R, uint32_t E, uint32_t a,
                                         uint32_t b0, uint32_t (&cnt)[CT_ROWS]) {
    if (first >= end) return;
    // one run ahead: the wave's next run's column value (a vector load), its CT_ROWS row values and the run index
    // after it (scalar loads) are in flight while the current run is counted. The look-ahead index is clamped to the
    // last run, so every load is of a valid row and the loop body has no branch.
    const uint32_t *__restrict__ row = pos + (size_t)perm[first] * E;
    uint32_t rn = perm[min(first + CT_WAVES, R - 1)];
    uint32_t ra = row[a], lb[CT_ROWS];
#pragma unroll
    for (uint32_t j = 0; j < CT_ROWS; ++j) lb[j] = row[FULL ? b0 + j : min(b0 + j, E - 1)];
    for (uint32_t i = first; i < end; i += CT_WAVES) {
        const uint32_t *__restrict__ rown = pos + (size_t)rn * E;
        uint32_t ran = rown[a];
        uint32_t lbn[CT_ROWS];
#pragma unroll
        for (uint32_t j = 0; j < CT_ROWS; ++j) lbn[j] = rown[FULL ? b0 + j : min(b0 + j, E - 1)];
        uint32_t rnn = perm[min(i + 2 * CT_WAVES, R - 1)];
        ra = ra == NMZ_NONE ? 0u : ra;  // an absent `a`: nothing is less than 0
        // the remapped value stays one register: left to itself the compiler folds the select into every compare
        // (v_cmp into an SGPR pair, s_and with the presence mask, SGPR-mask v_cndmask, add -- and spills SGPRs)
        asm("" : "+v"(ra));
#pragma unroll
        for (uint32_t j = 0; j < CT_ROWS; ++j) cnt[j] += lb[j] < ra ? 1u : 0u;  // an absent `b` is NMZ_NONE: never less
        // the look-ahead values are first needed here, behind the counting: without these the compiler rotates the
        // loop back and waits for every load right after issuing it (and nothing is scheduled across the barrier)
        __builtin_amdgcn_sched_barrier(0);
        asm volatile("" : "+v"(ran), "+s"(rnn));
        ra = ran;
        rn = rnn;
#pragma unroll
        for (uint32_t j = 0; j < CT_ROWS; ++j) {
            asm volatile("" : "+s"(lbn[j]));
            lb[j] = lbn[j];
        }
    }
}

template <bool FULL>
__global__ __launch_bounds__(TOPK_THREADS) void k_contrast_sweep(const uint32_t *__restrict__ pos,
                                                                  const uint32_t *__restrict__ perm, uint32_t R,
                                                                  uint32_t E, uint32_t tiles_a, uint32_t k,
                                                                  nmz_pair_counts *__restrict__ counts,
                                                                  nmz_topk_entry *__restrict__ lists,
                                                                  nmz_contrast_info *__restrict__ info) {
    __shared__ TopkShared sh;
    __shared__ uint32_t acc[CT_ROWS][CT_COLS];  // the tile's packed counters, summed over the waves
    __shared__ uint32_t wave_pos[CT_WAVES];
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // wave-uniform: the row loads stay scalar
    const uint32_t ta = blockIdx.x % tiles_a, tb = blockIdx.x / tiles_a;
    const uint32_t a = ta * CT_COLS + lane, b0 = tb * CT_ROWS;
    const uint32_t ac = min(a, E - 1);  // lanes past the last column read it again and are dropped below
    const uint32_t n_fail = info->n_fail, n_pass = info->n_pass;
    for (uint32_t i = threadIdx.x; i < CT_ROWS * CT_COLS; i += TOPK_THREADS) (&acc[0][0])[i] = 0;
    uint32_t cnt[CT_ROWS];
#pragma unroll
    for (uint32_t j = 0; j < CT_ROWS; ++j) cnt[j] = 0;
    ct_count<FULL>(pos, perm, w, n_fail, R, E, ac, b0, cnt);
#pragma unroll
    for (uint32_t j = 0; j < CT_ROWS; ++j) cnt[j] <<= 16;
    ct_count<FULL>(pos, perm, n_fail + w, R, R, E, ac, b0, cnt);
    __syncthreads();
    // F <= n_fail and P <= n_pass in total, so the sums of the packed words never carry from P into F
#pragma unroll
    for (uint32_t j = 0; j < CT_ROWS; ++j) atomicAdd(&acc[j][lane], cnt[j]);
    __syncthreads();

    // wave w takes rows 8 w .. 8 w + 7 of the tile: 2,048 pairs, one selection
    uint32_t n_pos = 0;
    nmz_topk_entry e[TOPK_PER_THREAD];
#pragma unroll
    for (uint32_t r = 0; r < TOPK_PER_THREAD; ++r) {
        const uint32_t j = w * TOPK_PER_THREAD + r, b = b0 + j;
        const uint32_t c2 = acc[j][lane];
        const uint32_t F = c2 >> 16, P = c2 & 0xffffu;
        e[r] = topk_sentinel();
        if (a < E && (FULL || b < E)) {
            if (counts) {
                nmz_pair_counts c;
                c.n_fail_with = F;
                c.n_pass_with = P;
                counts[(size_t)b * E + a] = c;
            }
            const int64_t score = (int64_t)((uint64_t)F * n_pass) - (int64_t)((uint64_t)P * n_fail);
            if (score > 0) {
                ++n_pos;
                e[r].seed = (uint64_t)b * E + a;
                e[r].sum_delay_ns = score * 65536 + (int64_t)F;
                e[r].n_fault = 0;
                e[r].first_fault = P;
            }
        }
    }
    if (k) topk_block_select<true>(e, k, lists + (uint64_t)blockIdx.x * k, sh);
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) n_pos += __shfl_xor(n_pos, o, 64);
    if (lane == 0) wave_pos[w] = n_pos;
    __syncthreads();
    if (threadIdx.x == 0) {
        n_pos = 0;
        for (uint32_t i = 0; i < CT_WAVES; ++i) n_pos += wave_pos[i];
        if (n_pos) atomicAdd(reinterpret_cast<unsigned long long *>(&info->n_positive), (unsigned long long)n_pos);
    }
}

// one wave per winner: the reverse direction's counts, then the record
__global__ __launch_bounds__(TOPK_THREADS) void k_contrast_pairs(const uint32_t *__restrict__ pos,
                                                                  const uint8_t *__restrict__ failed, uint32_t R,
                                                                  uint32_t E, uint32_t k,
                                                                  const nmz_topk_entry *__restrict__ tk,
                                                                  nmz_order_pair *__restrict__ pairs) {
    const uint32_t w = (blockIdx.x * TOPK_THREADS + threadIdx.x) >> 6, lane = threadIdx.x & 63;
    if (w >= k) return;
    const nmz_topk_entry x = tk[w];
    nmz_order_pair o;
    if (x.seed == UINT64_MAX) {  // past the positive pairs
        o.before = NMZ_NONE;
        o.after = NMZ_NONE;
        o.score = INT64_MIN;
        o.n_fail_with = o.n_pass_with = o.n_fail_against = o.n_pass_against = 0;
    } else {
        const uint32_t b = (uint32_t)(x.seed / E), a = (uint32_t)(x.seed % E);
        uint32_t fa = 0, pa = 0;
        for (uint32_t r = lane; r < R; r += 64) {
            const uint32_t pb = pos[(size_t)r * E + b], pp = pos[(size_t)r * E + a];
            const bool hit = pb != NMZ_NONE && pp != NMZ_NONE && pp < pb;
            const bool fl = failed[r] != 0;
            fa += hit && fl ? 1u : 0u;
            pa += hit && !fl ? 1u : 0u;
        }
#pragma unroll
        for (int s = 32; s >= 1; s >>= 1) {
            fa += __shfl_xor(fa, s, 64);
            pa += __shfl_xor(pa, s, 64);
        }
        o.before = b;
        o.after = a;
        o.score = x.sum_delay_ns >> 16;
        o.n_fail_with = (uint32_t)(x.sum_delay_ns & 0xffff);
        o.n_pass_with = x.first_fault;
        o.n_fail_against = fa;
        o.n_pass_against = pa;
    }
    if (lane == 0) pairs[w] = o;
}

// ---- host side -------------------------------------------------------------------------------------------------

// the limits that need no look at the arrays
static int contrast_limits(uint32_t R, uint32_t E) {
    NMZ_CHECK(E >= 1 && E <= CT_MAX_EVENTS, "n_events must be in [1, 4096]");
    NMZ_CHECK(R >= 1 && R <= CT_MAX_RUNS, "n_runs must be in [1, 65535]");
    return NMZ_OK;
}

// the labels, on the host: 0 or 1, and both present
static int contrast_labels(const uint8_t *failed, uint32_t R, uint32_t *n_fail) {
    uint32_t nf = 0;
    for (uint32_t r = 0; r < R; ++r) {
        NMZ_CHECK(failed[r] <= 1, "failed[" + std::to_string(r) + "] must be 0 or 1");
        nf += failed[r];
    }
    NMZ_CHECK(nf >= 1, "no failing run: nothing to contrast");
    NMZ_CHECK(nf < R, "no passing run: nothing to contrast");
    *n_fail = nf;
    return NMZ_OK;
}


// enqueue one contrast on st; scratch: SLOT_CONTRAST_RUN (the run order, the merged list, the per-workgroup lists)
static int contrast_run(nmz_ctx *ctx, hipStream_t st, const uint32_t *d_pos, const uint8_t *d_failed, uint32_t R,
                        uint32_t E, uint32_t k, nmz_pair_counts *d_counts, nmz_order_pair *d_pairs,
                        nmz_contrast_info *d_info) {
    NMZ_TRY(contrast_limits(R, E));
    NMZ_CHECK(k <= 256, "top-k supports k <= 256");
    NMZ_CHECK(d_pos && d_failed && d_info, "d_pos, d_failed or d_info is NULL");
    NMZ_CHECK(k == 0 || d_pairs, "d_pairs is NULL");
    const uint32_t tiles_a = ceil_div(E, CT_COLS), tiles_b = ceil_div(E, CT_ROWS);
    const uint64_t lists = (uint64_t)tiles_a * tiles_b;  // one per workgroup: at most 8,192
    uint32_t *d_perm;
    nmz_topk_entry *d_tk, *la, *lb;
    ScratchLayout lay;
    lay.add(&d_perm, R).add(&d_tk, k + 1).add(&la, lists * k + 1).add(&lb, lists * k + 1);
    NMZ_TRY(lay.bind(ctx->buf[SLOT_CONTRAST_RUN]));
    hipLaunchKernelGGL(k_contrast_runs, dim3(1), dim3(CT_RUNS_THREADS), 0, st, d_failed, R, d_perm, d_info);
    if (hipGetLastError() != hipSuccess) return fail(NMZ_EHIP, "k_contrast_runs launch failed");
    {
        KernelTimer kt(ctx, st, "contrast_sweep");
        const dim3 grid(tiles_a * tiles_b), block(TOPK_THREADS);
        if (E % CT_ROWS == 0)
            hipLaunchKernelGGL(k_contrast_sweep<true>, grid, block, 0, st, d_pos, d_perm, R, E, tiles_a, k, d_counts,
                               la, d_info);
        else  // the last tile's rows are clamped
            hipLaunchKernelGGL(k_contrast_sweep<false>, grid, block, 0, st, d_pos, d_perm, R, E, tiles_a, k, d_counts,
                               la, d_info);
        if (hipGetLastError() != hipSuccess) return fail(NMZ_EHIP, "k_contrast_sweep launch failed");
    }
    if (k == 0) return NMZ_OK;
    NMZ_TRY(topk_merge_lists(st, la, lb, lists, k, d_tk));
    hipLaunchKernelGGL(k_contrast_pairs, dim3(ceil_div((uint64_t)k * 64, TOPK_THREADS)), dim3(TOPK_THREADS), 0, st,
                       d_pos, d_failed, R, E, k, d_tk, d_pairs);
    if (hipGetLastError() != hipSuccess) return fail(NMZ_EHIP, "k_contrast_pairs launch failed");
    return NMZ_OK;
}

}  // namespace nmz

using namespace nmz;

extern "C" {

// One pair on the calling thread (naive.go:199-213 labels, summary.go:40-57): plain loops over the runs by the
// definition; no remap, no packed counter, nothing shared with the kernels.
int nmz_order_contrast_host(const uint32_t *pos, const uint8_t *failed, uint32_t n_runs, uint32_t n_events,
                            uint32_t before, uint32_t after, nmz_order_pair *out, nmz_contrast_info *info) {
    NMZ_TRY(contrast_limits(n_runs, n_events));
    NMZ_CHECK(pos && failed, "pos or failed is NULL");
    uint32_t n_fail = 0;
    NMZ_TRY(contrast_labels(failed, n_runs, &n_fail));
    NMZ_CHECK(before < n_events && after < n_events,
              "event index out of range (n_events = " + std::to_string(n_events) + ")");
    NMZ_CHECK(before != after, "before == after");
    const uint32_t n_pass = n_runs - n_fail;
    uint32_t fw = 0, pw = 0, fa = 0, pa = 0;
    for (uint32_t r = 0; r < n_runs; ++r) {
        const uint32_t pb = pos[(size_t)r * n_events + before], pp = pos[(size_t)r * n_events + after];
        if (pb == NMZ_NONE || pp == NMZ_NONE || pb == pp) continue;  // equal positions count for neither side
        if (pb < pp) {
            if (failed[r]) ++fw; else ++pw;
        } else {
            if (failed[r]) ++fa; else ++pa;
        }
    }
    if (out) {
        out->before = before;
        out->after = after;
        out->score = (int64_t)fw * (int64_t)n_pass - (int64_t)pw * (int64_t)n_fail;
        out->n_fail_with = fw;
        out->n_pass_with = pw;
        out->n_fail_against = fa;
        out->n_pass_against = pa;
    }
    if (info) {
        info->n_fail = n_fail;
        info->n_pass = n_pass;
        info->n_positive = 0;  // one pair says nothing about the others
    }
    return NMZ_OK;
}

int nmz_order_contrast_dev(nmz_ctx *ctx, const uint32_t *d_pos, const uint8_t *d_failed, uint32_t n_runs,
                           uint32_t n_events, uint32_t k, nmz_pair_counts *d_counts, nmz_order_pair *d_pairs,
                           nmz_contrast_info *d_info, void *stream) {
    NMZ_CHECK(ctx != nullptr, "ctx is NULL");
    CtxGuard g(ctx);
    NMZ_TRY(g.rc);
    return contrast_run(ctx, stream ? (hipStream_t)stream : ctx->stream, d_pos, d_failed, n_runs, n_events, k,
                        d_counts, d_pairs, d_info);
}

int nmz_order_contrast(nmz_ctx *ctx, const uint32_t *pos, const uint8_t *failed, uint32_t n_runs, uint32_t n_events,
                       uint32_t k, nmz_pair_counts *counts, nmz_order_pair *pairs, nmz_contrast_info *info) {
    // the arguments first: they are checked without a device
    NMZ_TRY(contrast_limits(n_runs, n_events));
    NMZ_CHECK(k <= 256, "top-k supports k <= 256");
    NMZ_CHECK(pos && failed, "pos or failed is NULL");
    uint32_t n_fail = 0;
    NMZ_TRY(contrast_labels(failed, n_runs, &n_fail));
    NMZ_CHECK(ctx != nullptr, "ctx is NULL");
    if (!pairs) k = 0;
    CtxGuard g(ctx);
    NMZ_TRY(g.rc);
    hipStream_t st = ctx->stream;
    nmz_contrast_info hinfo{};
    HostCall call(ctx);
    const size_t cells = (size_t)n_runs * n_events, sq = (size_t)n_events * n_events;
    uint32_t *d_pos;
    uint8_t *d_failed;
    nmz_pair_counts *d_counts;
    nmz_order_pair *d_pairs;
    nmz_contrast_info *d_info;
    ScratchLayout lay;
    lay.add(&d_pos, cells).add(&d_failed, n_runs).add(&d_counts, counts ? sq : 1).add(&d_pairs, k + 1).add(&d_info, 1);
    NMZ_TRY(lay.bind(ctx->buf[SLOT_CONTRAST_HOST]));
    NMZ_TRY(copy_h2d(d_pos, pos, cells, st));
    NMZ_TRY(copy_h2d(d_failed, failed, n_runs, st));
    NMZ_TRY(contrast_run(ctx, st, d_pos, d_failed, n_runs, n_events, k, counts ? d_counts : nullptr, d_pairs, d_info));
    if (counts) NMZ_TRY(copy_d2h(counts, d_counts, sq, st));
    NMZ_TRY(copy_d2h(pairs, d_pairs, k, st));
    NMZ_TRY(copy_d2h(&hinfo, d_info, 1, st));
    NMZ_TRY(call.done());
    if (info) *info = hinfo;
    return NMZ_OK;
}

// From the stored runs themselves (naive.go:235-257, historystorage.go:45 GetStoredHistory; labels naive.go:199-213):
// the CSR goes up, K7 (match.hip) makes pos on the device and the contrast reads it there. The rows are taken for
// the call from the context's pool, not from the contrast's scratch.
int nmz_order_contrast_runs(nmz_ctx *ctx, const uint64_t *sym, const int64_t *arrival_ns, uint32_t n_events,
                            const uint64_t *run_off, const uint64_t *run_sym, const uint8_t *failed, uint32_t n_runs,
                            uint32_t k, nmz_pair_counts *counts, nmz_order_pair *pairs, nmz_contrast_info *info) {
    // the arguments first: they are checked without a device
    NMZ_TRY(contrast_limits(n_runs, n_events));
    NMZ_CHECK(k <= 256, "top-k supports k <= 256");
    NMZ_TRY(match_validate(sym, arrival_ns, n_events, run_off, run_sym, n_runs));
    NMZ_CHECK(failed != nullptr, "failed is NULL");
    uint32_t n_fail = 0;
    NMZ_TRY(contrast_labels(failed, n_runs, &n_fail));
    NMZ_CHECK(ctx != nullptr, "ctx is NULL");
    if (!pairs) k = 0;
    CtxGuard g(ctx);
    NMZ_TRY(g.rc);
    hipStream_t st = ctx->stream;
    nmz_contrast_info hinfo{};
    HostCall call(ctx);
    const size_t sq = (size_t)n_events * n_events;
    uint8_t *d_failed;
    nmz_pair_counts *d_counts;
    nmz_order_pair *d_pairs;
    nmz_contrast_info *d_info;
    ScratchLayout lay;
    lay.add(&d_failed, n_runs).add(&d_counts, counts ? sq : 1).add(&d_pairs, k + 1).add(&d_info, 1);
    NMZ_TRY(lay.bind(ctx->buf[SLOT_CONTRAST_HOST]));
    uint32_t *d_pos = nullptr;
    NMZ_TRY(match_call(ctx, call, sym, arrival_ns, n_events, run_off, run_sym, n_runs, &d_pos));
    NMZ_TRY(copy_h2d(d_failed, failed, n_runs, st));
    NMZ_TRY(contrast_run(ctx, st, d_pos, d_failed, n_runs, n_events, k, counts ? d_counts : nullptr, d_pairs, d_info));
    if (counts) NMZ_TRY(copy_d2h(counts, d_counts, sq, st));
    NMZ_TRY(copy_d2h(pairs, d_pairs, k, st));
    NMZ_TRY(copy_d2h(&hinfo, d_info, 1, st));
    NMZ_TRY(call.done());
    if (info) *info = hinfo;
    return NMZ_OK;
}

}  // extern "C"
