// K3 -- banded Levenshtein over event-hash sequences + all-pairs k-NN.
//
// ED_w(a,b) = min(D(n,m), w+1), D restricted to |i-j| <= w (outside = +inf).
// Distance 0 <=> element-wise equal traces (SingleTrace.Equals,
// util/trace/trace.go:29-31); see DESIGN.md section 4.
//
// Fast path (k_ed_tile<W>), MI355X-first:
//  * symbols are remapped to dense 16-bit ids (exact: equality preserved);
//  * one lane per candidate trace b and TWO query traces (q1,q2) per wave,
//    packed in the lo/hi u16 halves of every register, so each packed VALU
//    op advances two DP cells; the band row (2W+1 cells) and a sliding window
//    of 2W+R candidate symbols live in VGPRs -- no cross-lane traffic, all 64
//    lanes busy (a wave-per-pair anti-diagonal mapping keeps at most w+1 of
//    64 lanes busy per step for w = 32);
//  * query symbols are wave-uniform scalar loads; candidate symbols come
//    from a lane-interleaved layout ([group][pos][64 lanes], one coalesced
//    128-B line per position), prefetched one row block ahead;
//  * Ukkonen cut-off: the band minimum of a row never decreases, so once it
//    exceeds W for both halves of every lane the wave stops (result W+1).
// Results go straight into per-trace top-k lists (u64 keys dist<<32|id,
// cascade atomicMin insertion: lock-free and order-independent).
//
// Generic path (k_ed_generic): one thread per pair, any band, u64 symbols,
// band row in global scratch. Used for nmz_ed_pairs and as the fallback.
#include <algorithm>

#include "ed_generic_dev.h"
#include "ed_knn_dev.h"
#include "ed_plan.h"

namespace nmz {

typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));

constexpr uint16_t QUERY_PAD = 0xfffe; // query symbol past its end
constexpr uint16_t INF16 = 0x7f00;     // +inf for u16 DP cells (grows by < W before leaving the band)
constexpr int ED_R = 8;                // rows per unrolled block

__device__ __forceinline__ u16x2 pk_min(u16x2 a, u16x2 b) { return __builtin_elementwise_min(a, b); }
__device__ __forceinline__ u16x2 splat(uint16_t v) { return u16x2{v, v}; }
__device__ __forceinline__ u16x2 as_pk(uint32_t v) { return __builtin_bit_cast(u16x2, v); }
__device__ __forceinline__ uint32_t as_u32(u16x2 v) { return __builtin_bit_cast(uint32_t, v); }

// ---------------------------------------------------------------------------
// wave -> (query pair, candidate group) over the upper triangle of 64x64 blocks
//   block b (queries 64b..64b+63 = 32 query pairs) x groups g in [b, G)
//   waves in block b: 32*(G-b); inner order keeps one candidate group for
//   32 consecutive waves (8 workgroups) so the group's symbols are re-read
//   from the same L2.
// ---------------------------------------------------------------------------
__host__ __device__ inline uint64_t tri_prefix(uint64_t b, uint64_t G) { return 32 * (b * G - b * (b - 1) / 2); }

struct EdArgs {
    const uint16_t *qsym;       // query symbols, CSR order
    const uint64_t *qoff;       // [N+1]
    const uint16_t *csym;       // candidate symbols, [group][pos][64]
    const uint64_t *coff;       // [G] element offset of each group block
    const uint32_t *gmax;       // [G] padded length of each group
    const uint32_t *len;        // [N]
    uint32_t N, G, k;
    uint64_t n_waves;           // waves of this shard
    uint32_t shard, n_shards;   // 32-wave groups dealt round-robin over shards
    uint64_t *knn;              // [N][k]
};

template <int W>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2))) void k_ed_tile(EdArgs A) {
    // at least two waves per SIMD: at W = 32 the compiler's own allocation was 256 VGPRs + 26 AGPRs (one wave); bound
    // to 256 it spills ~23 VGPRs (the row-block size R = 2, 4, 8 changes nothing)
    constexpr int R = ED_R;
    constexpr int NB = 2 * W + 1;       // band cells
    constexpr int NW = 2 * W + R;       // window symbols
    // XCD-aware: hardware block b runs on XCD b%8; give each XCD a contiguous
    // range of logical blocks so waves sharing a candidate group share an L2.
    const uint32_t nblk = gridDim.x, per_xcd = nblk / 8;
    const uint32_t hb = blockIdx.x;
    const uint32_t lb = (hb % 8) * per_xcd + hb / 8;
    const uint64_t lwave = (uint64_t)lb * 4 + (threadIdx.x >> 6);
    const uint32_t lane = threadIdx.x & 63;
    if (lwave >= A.n_waves) return;
    const uint64_t wave = ((lwave / 32) * A.n_shards + A.shard) * 32 + lwave % 32;

    // locate block b: largest b with tri_prefix(b) <= wave
    uint32_t lo = 0, hi = A.G;
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) / 2;
        if (tri_prefix(mid, A.G) <= wave) lo = mid; else hi = mid;
    }
    const uint32_t b = lo;
    const uint64_t idx = wave - tri_prefix(b, A.G);
    const uint32_t g = b + (uint32_t)(idx / 32);
    const uint32_t q1 = 64 * b + 2 * (uint32_t)(idx % 32), q2 = q1 + 1;
    const uint32_t j = 64 * g + lane;

    const bool v1 = q1 < A.N && j < A.N && j > q1;
    const bool v2 = q2 < A.N && j < A.N && j > q2;
    const uint32_t n1 = q1 < A.N ? A.len[q1] : 0, n2 = q2 < A.N ? A.len[q2] : 0;
    const uint32_t m = j < A.N ? A.len[j] : 0;
    const uint16_t *__restrict__ a1 = A.qsym + (q1 < A.N ? A.qoff[q1] : 0);
    const uint16_t *__restrict__ a2 = A.qsym + (q2 < A.N ? A.qoff[q2] : 0);
    const uint16_t *__restrict__ cs = A.csym + A.coff[g] + lane;
    const uint32_t glen = A.gmax[g];

    // per-half state: result, whether still running
    uint32_t r1 = W + 1, r2 = W + 1;
    bool run1 = v1, run2 = v2;
    const int32_t d1 = (int32_t)m - (int32_t)n1, d2 = (int32_t)m - (int32_t)n2;
    if (run1 && (d1 > W || d1 < -W)) run1 = false;  // |n-m| > W: W+1
    if (run2 && (d2 > W || d2 < -W)) run2 = false;
    if (run1 && n1 == 0) { r1 = m; run1 = false; }
    if (run2 && n2 == 0) { r2 = m; run2 = false; }

    const uint32_t nrows = __builtin_amdgcn_readfirstlane(max(n1, n2));  // n_h = 0 for q_h >= N
    u16x2 D[NB];
    uint32_t win[NW];  // packed (b, b) symbols for window positions i0-W .. i0-W+NW-1
#pragma unroll
    for (int t = 0; t < NB; ++t) D[t] = splat(t >= W ? (uint16_t)(t - W) : INF16);
    auto load_sym = [&](int64_t pos) -> uint32_t {
        const uint32_t s = (pos >= 0 && pos < (int64_t)glen) ? (uint32_t)cs[(uint64_t)pos * 64] : (uint32_t)CAND_PAD;
        return s | (s << 16);
    };
#pragma unroll
    for (int t = 0; t < NW; ++t) win[t] = load_sym((int64_t)t - W);

    const u16x2 one = splat(1);
    uint32_t i0 = 0;
    const bool any_run = __builtin_amdgcn_readfirstlane((uint32_t)__any(run1 || run2)) != 0;
    if (any_run) {
        while (i0 < nrows) {
            // next extraction row for the halves that are still alive
            const uint32_t stop = min(nrows, min(n1 > i0 ? n1 : nrows, n2 > i0 ? n2 : nrows));
            const uint32_t stop_u = __builtin_amdgcn_readfirstlane(stop);
            if (i0 + R <= stop_u) {
                // prefetch the symbols entering the window after this block
                uint32_t nxt[R];
#pragma unroll
                for (int r = 0; r < R; ++r) nxt[r] = load_sym((int64_t)i0 - W + NW + r);
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    const uint32_t i = i0 + r;  // computing row i+1, symbols a[i]
                    const uint32_t s1 = i < n1 ? a1[i] : QUERY_PAD, s2 = i < n2 ? a2[i] : QUERY_PAD;
                    const uint32_t ap = __builtin_amdgcn_readfirstlane(s1 | (s2 << 16));
                    u16x2 left = splat(INF16);
#pragma unroll
                    for (int t = 0; t < NB; ++t) {
                        const u16x2 c = pk_min(as_pk(win[r + t] ^ ap), one);
                        const u16x2 diag = D[t] + c;
                        const u16x2 up = (t + 1 < NB) ? D[t + 1] : splat(INF16);
                        const u16x2 nd = pk_min(diag, pk_min(up, left) + one);
                        D[t] = nd;
                        left = nd;
                    }
                }
#pragma unroll
                for (int t = 0; t < NW - R; ++t) win[t] = win[t + R];
#pragma unroll
                for (int r = 0; r < R; ++r) win[NW - R + r] = nxt[r];
                i0 += R;
            } else {
                // single row (lands exactly on an extraction row)
                const uint32_t i = i0;
                const uint32_t s1 = i < n1 ? a1[i] : QUERY_PAD, s2 = i < n2 ? a2[i] : QUERY_PAD;
                const uint32_t ap = __builtin_amdgcn_readfirstlane(s1 | (s2 << 16));
                u16x2 left = splat(INF16);
#pragma unroll
                for (int t = 0; t < NB; ++t) {
                    const u16x2 c = pk_min(as_pk(win[t] ^ ap), one);
                    const u16x2 diag = D[t] + c;
                    const u16x2 up = (t + 1 < NB) ? D[t + 1] : splat(INF16);
                    const u16x2 nd = pk_min(diag, pk_min(up, left) + one);
                    D[t] = nd;
                    left = nd;
                }
                const uint32_t nx = load_sym((int64_t)i0 - W + NW);
#pragma unroll
                for (int t = 0; t < NW - 1; ++t) win[t] = win[t + 1];
                win[NW - 1] = nx;
                i0 += 1;
            }
            // extraction at row n_h: D(n, m) sits on diagonal m - n
            if (i0 == n1 && run1) {
                uint32_t v = W + 1;
#pragma unroll
                for (int t = 0; t < NB; ++t) v = (t - W == d1) ? (uint32_t)D[t].x : v;
                r1 = min(v, (uint32_t)W + 1);
                run1 = false;
            }
            if (i0 == n2 && run2) {
                uint32_t v = W + 1;
#pragma unroll
                for (int t = 0; t < NB; ++t) v = (t - W == d2) ? (uint32_t)D[t].y : v;
                r2 = min(v, (uint32_t)W + 1);
                run2 = false;
            }
            // cut-off: row band minimum > W stays > W
            if ((i0 & 15) == 0 || !(run1 || run2)) {
                u16x2 mn = D[0];
#pragma unroll
                for (int t = 1; t < NB; ++t) mn = pk_min(mn, D[t]);
                if (mn.x > W) run1 = false;
                if (mn.y > W) run2 = false;
                if (!__any(run1 || run2)) break;
            }
        }
    }
    // publish: candidate lists (per lane) and query lists (wave-reduced)
    const uint64_t key1 = v1 ? (((uint64_t)r1 << 32) | j) : UINT64_MAX;
    const uint64_t key2 = v2 ? (((uint64_t)r2 << 32) | j) : UINT64_MAX;
    if (v1) knn_insert(A.knn + (uint64_t)j * A.k, A.k, ((uint64_t)r1 << 32) | q1);
    if (v2) knn_insert(A.knn + (uint64_t)j * A.k, A.k, ((uint64_t)r2 << 32) | q2);
    if (q1 < A.N) knn_insert_wave(A.knn + (uint64_t)q1 * A.k, A.k, key1, lane);
    if (q2 < A.N) knn_insert_wave(A.knn + (uint64_t)q2 * A.k, A.k, key2, lane);
}

// ---------------------------------------------------------------------------
// generic: one thread per pair, u64 symbols, band row in global scratch
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_ed_generic(const uint64_t *__restrict__ off, const uint64_t *__restrict__ sym,
                                                    const uint32_t *__restrict__ pairs, uint64_t n_pairs, uint32_t W,
                                                    uint32_t *__restrict__ scratch, uint32_t *__restrict__ dist) {
    const uint64_t nthr = (uint64_t)gridDim.x * blockDim.x;
    const uint64_t tid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (uint64_t p = tid; p < n_pairs; p += nthr) {
        const uint32_t ia = pairs[2 * p], ib = pairs[2 * p + 1];
        dist[p] = generic_band_dist(sym + off[ia], (int64_t)(off[ia + 1] - off[ia]), sym + off[ib],
                                    (int64_t)(off[ib + 1] - off[ib]), W, scratch + tid, nthr);
    }
}

__global__ void k_knn_init(uint64_t *knn, uint64_t n) {
    uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) knn[i] = UINT64_MAX;
}

// a search's start: its k-NN lists and (bit-parallel plans) the work counters in one launch (a separate memset of
// the counters was one more queue entry per search, ~5 us: a shard of a sharded search pays it once per shard)
__global__ void k_knn_init_cnt(uint64_t *knn, uint64_t n, uint64_t *counters, uint32_t n_cnt) {
    uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) knn[i] = UINT64_MAX;
    if (counters && i < n_cnt) counters[i] = 0;
}

__global__ void k_knn_final(const uint64_t *__restrict__ knn, uint64_t n, uint32_t *__restrict__ ids,
                            uint32_t *__restrict__ ds) {
    uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint64_t key = knn[i];
    ids[i] = key == UINT64_MAX ? NMZ_NONE : (uint32_t)key;
    ds[i] = key == UINT64_MAX ? NMZ_NONE : (uint32_t)(key >> 32);
}

// Complete k-NN lists whose listed keys are the results within the band (dist < fill_d): every pair not listed has
// the result fill_d = band + 1, so list i takes (fill_d, j) for the smallest ids j < n_cand not listed (j != i when
// self_exclude), in increasing j, until it holds k keys (UINT64_MAX where fewer candidates exist). Keys at or
// above fill_d already in the list (kernels that list every pair) are recomputed to the same values.
__global__ void k_knn_fill(uint64_t *knn, uint32_t n_lists, uint32_t k, uint32_t n_cand, uint32_t fill_d,
                           int self_exclude) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_lists) return;
    uint64_t *L = knn + (uint64_t)i * k;
    uint32_t c = 0;
    while (c < k && L[c] != UINT64_MAX && (uint32_t)(L[c] >> 32) < fill_d) ++c;
    uint32_t j = 0;
    for (uint32_t s = c; s < k; ++s) {
        for (;; ++j) {
            if (j >= n_cand) break;
            if (self_exclude && j == i) continue;
            bool listed = false;
            for (uint32_t t = 0; t < c; ++t) listed |= (uint32_t)L[t] == j;
            if (!listed) break;
        }
        L[s] = j < n_cand ? (((uint64_t)fill_d << 32) | j) : UINT64_MAX;
        ++j;
    }
}

// all-pairs via the generic kernel (fallback): pair list = upper triangle
__global__ void k_pairs_upper(uint32_t N, uint64_t start, uint64_t count, uint32_t *pairs) {
    uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= count) return;
    uint64_t p = start + t;  // p-th pair (i<j), row-major
    // i = largest with i*(2N-i-1)/2 <= p
    double Nd = N;
    uint64_t i = (uint64_t)floor(((2 * Nd - 1) - sqrt((2 * Nd - 1) * (2 * Nd - 1) - 8.0 * (double)p)) / 2);
    auto base = [&](uint64_t r) { return r * (2 * (uint64_t)N - r - 1) / 2; };
    while (i > 0 && base(i) > p) --i;
    while (base(i + 1) <= p) ++i;
    const uint64_t jj = i + 1 + (p - base(i));
    pairs[2 * t] = (uint32_t)i;
    pairs[2 * t + 1] = (uint32_t)jj;
}

__global__ void k_knn_from_pairs(const uint32_t *__restrict__ pairs, const uint32_t *__restrict__ dist, uint64_t count,
                                 uint64_t *knn, uint32_t k) {
    uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= count) return;
    const uint32_t i = pairs[2 * t], j = pairs[2 * t + 1];
    const uint64_t d = dist[t];
    knn_insert(knn + (uint64_t)i * k, k, (d << 32) | j);
    knn_insert(knn + (uint64_t)j * k, k, (d << 32) | i);
}

void knn_init_launch(uint64_t *knn, uint64_t n, hipStream_t st) {
    hipLaunchKernelGGL(k_knn_init, dim3(ceil_div(n, 256)), dim3(256), 0, st, knn, n);
}

void knn_fill_launch(uint64_t *knn, uint32_t n_lists, uint32_t k, uint32_t n_cand, uint32_t fill_d, int self_exclude,
                     hipStream_t st) {
    hipLaunchKernelGGL(k_knn_fill, dim3(ceil_div(n_lists, 256)), dim3(256), 0, st, knn, n_lists, k, n_cand, fill_d,
                       self_exclude);
}

int knn_final_to_host(HostCall &call, const uint64_t *knn, uint64_t n, uint32_t *d_id, uint32_t *d_ds,
                      uint32_t *knn_id, uint32_t *knn_dist) {
    hipLaunchKernelGGL(k_knn_final, dim3(ceil_div(n, 256)), dim3(256), 0, call.st, knn, n, d_id, d_ds);
    NMZ_HIP(hipGetLastError());
    if (knn_id) NMZ_TRY(copy_d2h(knn_id, d_id, n, call.st));
    if (knn_dist) NMZ_TRY(copy_d2h(knn_dist, d_ds, n, call.st));
    return call.done();
}

static int ed_knn_run(nmz_ed_plan *p, hipStream_t st, uint32_t k, uint64_t *d_knn, uint32_t shard = 0,
                      uint32_t n_shards = 1) {
    const uint32_t N = p->n;
    if (N == 0 || k == 0) return NMZ_OK;
    {
        uint64_t *cnt = p->bv ? p->d_counters : nullptr;  // zeroed with the lists (was a memset per search)
        const uint64_t nl = (uint64_t)N * k, nt = std::max<uint64_t>(nl, cnt ? ED_CNT_WORDS : 0);
        hipLaunchKernelGGL(k_knn_init_cnt, dim3(ceil_div(nt, 256)), dim3(256), 0, st, d_knn, nl, cnt,
                           (uint32_t)ED_CNT_WORDS);
    }
    if (p->wide) {
        EdWideArgs A = ed_wide_plan_args(p, k);
        A.knn = d_knn;
        A.n_pairs = (uint64_t)N * (N - 1) / 2;
        const uint64_t chunks = (A.n_pairs + 31) / 32;
        A.n_waves = (shard < chunks ? (chunks - shard + n_shards - 1) / n_shards : 0) * 32;
        A.shard = shard;
        A.n_shards = n_shards;
        if (A.n_waves == 0) return NMZ_OK;
        KernelTimer kt(p->ctx, st, "ed_wide");
        return ed_wide_launch(A, p->ww, st);
    }
    if (p->bv) {
        EdBvArgs A;
        A.bsym = p->d_bsym;
        A.soff = p->d_soff;
        A.len = p->d_len;
        A.chunk_start = p->d_chunk_start;
        A.knn = d_knn;
        A.counters = p->d_counters;
        A.prof = p->qgram ? (const uint4 *)p->d_prof : nullptr;
        A.N = N;
        A.G = p->G;
        A.k = k;
        A.lds_dw = p->lds_dw;
        A.pool = p->pool;
        A.w = p->band;
        A.rmap_dw = p->rmap_dw;
        A.claim_dw = p->claim_dw;
        A.row_bytes = p->row_bytes;
        A.shard = shard;
        A.n_shards = n_shards;
        int rc = 1;
        if (A.prof && p->two_phase) {  // filter tiles + DP work items (the search's "ed_bv" time)
            KernelTimer kt(p->ctx, st, "ed_bv");
            rc = ed_bv_two_phase(p, st, A, d_knn);
            if (rc < 0) return rc;
        }
        if (rc == 1) {  // the single-kernel search (no q-gram filter, or N >= 2^30): a plan-wide choice
            // every (row, chunk) of the plan is launched; a workgroup whose query block this shard does not own
            // (ed_block_shard, the two-phase search's rule) exits at once, so a shard owns the same pairs whichever
            // form of the search its plan took
            A.n_chunks = p->n_chunks;
            if (A.n_chunks > 0) {
                A.rq = p->rq;
                uint64_t blocks = A.n_chunks * (p->rq / 2);
                blocks = (blocks + 7) / 8 * 8;
                NMZ_CHECK(blocks < (1ULL << 31), "too many traces for one launch");
                NMZ_HIP(hipMemsetAsync(p->d_counters, 0, ED_CNT_WORDS * 8, st));
                KernelTimer kt(p->ctx, st, "ed_bv");
                NMZ_TRY(ed_bv_launch(A, p->bw, p->cmp, blocks, st));
            }
        }
        // k_ed_bv lists in-band results only; a shard's partial lists are completed after the merge
        // (nmz_ed_knn_fill_dev)
        if (n_shards == 1) {
            knn_fill_launch(d_knn, N, k, N, p->band + 1, 1, st);
            NMZ_HIP(hipGetLastError());
        }
        return NMZ_OK;
    }
    if (p->fast) {
        EdArgs A;
        A.qsym = p->d_qsym;
        A.qoff = p->d_qoff;
        A.csym = p->d_csym;
        A.coff = p->d_coff;
        A.gmax = p->d_gmax;
        A.len = p->d_len;
        A.N = N;
        A.G = p->G;
        A.k = k;
        A.knn = d_knn;
        const uint64_t groups = tri_prefix(p->G, p->G) / 32;
        A.shard = shard;
        A.n_shards = n_shards;
        A.n_waves = (shard < groups ? (groups - shard + n_shards - 1) / n_shards : 0) * 32;
        if (A.n_waves == 0) return NMZ_OK;
        uint64_t blocks = (A.n_waves + 3) / 4;
        blocks = (blocks + 7) / 8 * 8;  // multiple of 8 for the XCD remap
        NMZ_CHECK(blocks < (1ULL << 31), "too many traces for one launch");
        KernelTimer kt(p->ctx, st, "ed_tile");
        switch (p->band) {
            case 8: hipLaunchKernelGGL(k_ed_tile<8>, dim3((unsigned)blocks), dim3(256), 0, st, A); break;
            case 16: hipLaunchKernelGGL(k_ed_tile<16>, dim3((unsigned)blocks), dim3(256), 0, st, A); break;
            case 32: hipLaunchKernelGGL(k_ed_tile<32>, dim3((unsigned)blocks), dim3(256), 0, st, A); break;
            default: return fail(NMZ_EINVAL, "internal: band has no fast kernel");
        }
        NMZ_HIP(hipGetLastError());
        return NMZ_OK;
    }
    // generic fallback: upper-triangle pair list in chunks
    const uint64_t total_pairs = (uint64_t)N * (N - 1) / 2;
    const uint64_t chunk = std::min<uint64_t>(total_pairs, 1ULL << 22);
    const unsigned gthreads = 256 * 1024;
    uint32_t *d_pairs, *d_dist, *d_row;
    ScratchLayout lay;
    lay.add(&d_pairs, chunk * 2 + 1).add(&d_dist, chunk + 1).add(&d_row, (uint64_t)(2 * p->band + 1) * gthreads);
    NMZ_TRY(lay.bind(p->ctx->buf[SLOT_ED_KNN]));
    for (uint64_t s = (uint64_t)shard * chunk; s < total_pairs; s += (uint64_t)n_shards * chunk) {
        const uint64_t c = std::min(chunk, total_pairs - s);
        hipLaunchKernelGGL(k_pairs_upper, dim3(ceil_div(c, 256)), dim3(256), 0, st, N, s, c, d_pairs);
        hipLaunchKernelGGL(k_ed_generic, dim3(gthreads / 256), dim3(256), 0, st, p->d_off64, p->d_sym64, d_pairs, c,
                           p->band, d_row, d_dist);
        hipLaunchKernelGGL(k_knn_from_pairs, dim3(ceil_div(c, 256)), dim3(256), 0, st, d_pairs, d_dist, c, d_knn, k);
    }
    NMZ_HIP(hipGetLastError());
    return NMZ_OK;
}

}  // namespace nmz

using namespace nmz;

extern "C" {

int nmz_ed_plan_create(nmz_ctx *ctx, const uint64_t *off, const uint64_t *sym, uint32_t n_traces, uint32_t band,
                       nmz_ed_plan **out) {
    return nmz_ed_plan_create_opts(ctx, off, sym, nullptr, n_traces, band, 0, out);
}

int nmz_ed_plan_destroy(nmz_ed_plan *plan) {
    if (!plan) return NMZ_OK;
    CtxGuard g(plan->ctx);
    ed_plan_release(plan);
    return NMZ_OK;
}

int nmz_ed_plan_is_fast(const nmz_ed_plan *plan) {
    if (!plan) return 0;
    return plan->wide ? 3 : (plan->bv ? 2 : (plan->fast ? 1 : 0));
}

int nmz_ed_plan_counters(nmz_ed_plan *plan, uint64_t *out, void *stream) {
    NMZ_CHECK(plan != nullptr && out != nullptr, "NULL argument");
    for (int i = 0; i < NMZ_ED_NCOUNTERS; ++i) out[i] = 0;
    if (!plan->d_counters) return NMZ_OK;
    static_assert(ED_BV_NCOUNTERS == NMZ_ED_NCOUNTERS, "counter layout");
    CtxGuard g(plan->ctx);
    hipStream_t st = stream ? (hipStream_t)stream : plan->ctx->stream;
    std::vector<uint64_t> lines(ED_CNT_WORDS);
    NMZ_HIP(hipMemcpyAsync(lines.data(), plan->d_counters, ED_CNT_WORDS * 8, hipMemcpyDeviceToHost, st));
    NMZ_HIP(hipStreamSynchronize(st));
    for (uint32_t sidx = 0; sidx < ED_CNT_STRIPES; ++sidx)
        for (int i = 0; i < ED_BV_NCOUNTERS; ++i) out[i] += lines[sidx * ED_CNT_LINE + i];
    return ed_tp_flag_check(plan, true, st);
}

int nmz_ed_plan_create_dev(nmz_ctx *ctx, const uint64_t *off, const uint64_t *d_sym, uint32_t n_traces,
                           uint32_t band, nmz_ed_plan **out) {
    NMZ_CHECK(ctx != nullptr, "ctx is NULL");
    NMZ_CHECK(n_traces == 0 || off, "off is NULL");
    NMZ_CHECK(n_traces == 0 || off[n_traces] == 0 || d_sym, "d_sym is NULL");
    return nmz_ed_plan_create_opts(ctx, off, nullptr, d_sym, n_traces, band, 0, out);
}

int nmz_ed_plan_create_opts(nmz_ctx *ctx, const uint64_t *off, const uint64_t *sym, const uint64_t *d_sym,
                            uint32_t n_traces, uint32_t band, uint32_t opts, nmz_ed_plan **out) {
    NMZ_CHECK(ctx != nullptr, "ctx is NULL");
    NMZ_CHECK(n_traces == 0 || off, "off is NULL");
    NMZ_CHECK(!(sym && d_sym), "pass sym (host) or d_sym (device), not both");
    CtxGuard g(ctx);
    NMZ_TRY(g.rc);
    return ed_plan_build(ctx, off, sym, n_traces, band, out, d_sym, opts);
}

int nmz_ed_plan_fingerprint(const nmz_ed_plan *p, uint64_t *fp) {
    NMZ_CHECK(p != nullptr && fp != nullptr, "NULL argument");
    const uint64_t kind = p->wide ? 3 : (p->bv ? 2 : (p->fast ? 1 : 0));
    fp[0] = NMZ_ED_FP_VERSION;
    fp[1] = kind | (uint64_t)p->band << 8 | (uint64_t)(p->bv ? p->bw : p->ww) << 40;
    fp[2] = p->n;
    fp[3] = p->total;
    fp[4] = (uint64_t)p->two_phase | (uint64_t)p->qgram << 1 | (uint64_t)p->cmp << 2;
    fp[5] = (uint64_t)p->rq | (uint64_t)p->pool << 32;
    fp[6] = p->off_hash;
    fp[7] = p->n_sym;
    return NMZ_OK;
}

int nmz_ed_allpairs_knn_dev(nmz_ed_plan *plan, uint32_t k, uint64_t *d_knn_keys, void *stream) {
    return nmz_ed_allpairs_knn_shard_dev(plan, k, 0, 1, d_knn_keys, stream);
}

uint32_t nmz_ed_block_shard(uint32_t qb, uint32_t n_shards) { return ed_block_shard(qb, n_shards); }

int nmz_ed_allpairs_knn_shard_dev(nmz_ed_plan *plan, uint32_t k, uint32_t shard, uint32_t n_shards,
                                  uint64_t *d_knn_keys, void *stream) {
    NMZ_CHECK(plan != nullptr, "plan is NULL");
    NMZ_CHECK(k >= 1 && k <= 64, "k must be in [1, 64]");
    NMZ_CHECK(n_shards >= 1 && shard < n_shards, "bad shard");
    CtxGuard g(plan->ctx);
    NMZ_TRY(g.rc);
    return ed_knn_run(plan, stream ? (hipStream_t)stream : plan->ctx->stream, k, d_knn_keys, shard, n_shards);
}

// merge n_parts partial k-NN key lists ([n_parts][N][k], each sorted) into [N][k]
__global__ void k_knn_merge(const uint64_t *__restrict__ parts, uint32_t n_parts, uint32_t N, uint32_t k,
                            uint64_t *__restrict__ out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    uint32_t pos[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (uint32_t s = 0; s < k; ++s) {
        uint64_t best = UINT64_MAX;
        uint32_t bp = 0;
        for (uint32_t p = 0; p < n_parts; ++p) {
            const uint64_t v = pos[p] < k ? parts[((uint64_t)p * N + i) * k + pos[p]] : UINT64_MAX;
            if (v < best) {
                best = v;
                bp = p;
            }
        }
        if (best != UINT64_MAX) pos[bp]++;
        out[(uint64_t)i * k + s] = best;
    }
}

int nmz_knn_merge_dev(nmz_ctx *ctx, const uint64_t *d_parts, uint32_t n_parts, uint32_t n_traces, uint32_t k,
                      uint64_t *d_out, void *stream) {
    NMZ_CHECK(ctx != nullptr, "ctx is NULL");
    NMZ_CHECK(n_parts >= 1 && n_parts <= 8, "n_parts must be in [1, 8]");
    CtxGuard g(ctx);
    NMZ_TRY(g.rc);
    if (n_traces == 0 || k == 0) return NMZ_OK;
    hipLaunchKernelGGL(k_knn_merge, dim3(ceil_div(n_traces, 256)), dim3(256), 0,
                       stream ? (hipStream_t)stream : ctx->stream, d_parts, n_parts, n_traces, k, d_out);
    NMZ_HIP(hipGetLastError());
    return NMZ_OK;
}

int nmz_ed_knn_fill_dev(nmz_ed_plan *plan, uint32_t k, uint64_t *d_knn_keys, void *stream) {
    NMZ_CHECK(plan != nullptr, "plan is NULL");
    NMZ_CHECK(k >= 1 && k <= 64, "k must be in [1, 64]");
    CtxGuard g(plan->ctx);
    NMZ_TRY(g.rc);
    if (plan->n == 0) return NMZ_OK;
    NMZ_CHECK(d_knn_keys != nullptr, "d_knn_keys is NULL");
    knn_fill_launch(d_knn_keys, plan->n, k, plan->n, plan->band + 1, 1,
                    stream ? (hipStream_t)stream : plan->ctx->stream);
    NMZ_HIP(hipGetLastError());
    return NMZ_OK;
}

int nmz_ed_allpairs_knn(nmz_ctx *ctx, const uint64_t *off, const uint64_t *sym, uint32_t n_traces, uint32_t band,
                        uint32_t k, uint32_t *knn_id, uint32_t *knn_dist) {
    NMZ_CHECK(ctx != nullptr, "ctx is NULL");
    NMZ_CHECK(k <= 64, "k must be <= 64");
    CtxGuard g(ctx);
    NMZ_TRY(g.rc);
    if (n_traces == 0 || k == 0) return NMZ_OK;
    nmz_ed_plan *plan = nullptr;
    NMZ_TRY(ed_plan_build(ctx, off, sym, n_traces, band, &plan));
    EdPlanPtr owner(plan);
    HostCall call(ctx);  // behind owner: the plan goes after the drain
    const uint64_t nk = (uint64_t)n_traces * k;
    uint64_t *d_knn;
    uint32_t *d_id, *d_ds;
    ScratchLayout lay;
    lay.add(&d_knn, nk).add(&d_id, nk).add(&d_ds, nk);
    NMZ_TRY(lay.bind(ctx->buf[SLOT_ED_KNN_HOST]));
    NMZ_TRY(ed_knn_run(plan, call.st, k, d_knn));
    return knn_final_to_host(call, d_knn, nk, d_id, d_ds, knn_id, knn_dist);
}

int nmz_ed_pairs(nmz_ctx *ctx, const uint64_t *off, const uint64_t *sym, uint32_t n_traces, const uint32_t *pairs,
                 uint64_t n_pairs, uint32_t band, uint32_t *dist) {
    NMZ_CHECK(ctx != nullptr, "ctx is NULL");
    NMZ_CHECK(band < (1u << 20), "band too large");
    CtxGuard g(ctx);
    NMZ_TRY(g.rc);
    if (n_pairs == 0) return NMZ_OK;
    NMZ_CHECK(pairs && dist && off, "NULL argument");
    for (uint64_t t = 0; t < 2 * n_pairs; ++t) NMZ_CHECK(pairs[t] < n_traces, "pair index out of range");
    hipStream_t st = ctx->stream;
    HostCall call(ctx);
    // n_pairs > 0 and every pair index is below n_traces, so there is a trace and off[n_traces] is the total
    const uint64_t total = off[n_traces];
    const unsigned gthreads = (unsigned)std::min<uint64_t>(256 * 1024, (n_pairs + 255) / 256 * 256);
    uint64_t *d_off, *d_sym;
    uint32_t *d_pairs, *d_dist, *d_row;
    ScratchLayout lay;
    lay.add(&d_off, n_traces + 1).add(&d_sym, total + 1).add(&d_pairs, 2 * n_pairs).add(&d_dist, n_pairs);
    lay.add(&d_row, (uint64_t)(2 * band + 1) * gthreads);
    NMZ_TRY(lay.bind(ctx->buf[SLOT_ED_PAIRS_HOST]));
    NMZ_TRY(upload_csr(d_off, d_sym, off, sym, n_traces, st));
    NMZ_TRY(copy_h2d(d_pairs, pairs, 2 * n_pairs, st));
    hipLaunchKernelGGL(k_ed_generic, dim3(gthreads / 256), dim3(256), 0, st, d_off, d_sym, d_pairs, n_pairs, band, d_row,
                       d_dist);
    NMZ_HIP(hipGetLastError());
    NMZ_TRY(copy_d2h(dist, d_dist, n_pairs, st));
    return call.done();
}

}  // extern "C"
