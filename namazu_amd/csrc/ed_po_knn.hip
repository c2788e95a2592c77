// K11 -- PO k-NN search: the k nearest stored runs by per-entity edit distance
// (historystorage/historystorage.go:50-51 is the search interface this extends, naive/naive.go:235-257 the
// reference's equality search, cli/tools/visualize.go:62-136 createTracesPerEntity / tracesEqualInPO: d == 0 <=>
// tracesEqualInPO).
//
// The semantics are DESIGN.md section 2, "PO k-NN search": d(q, c) = ED^PO_w(query q, stored c) = min(sum over the
// entities g of Lev(q|g, c|g), w + 1) as section 2 "Edit scripts per entity" defines it; per query the k smallest keys
// d << 32 | c over the stored c != q_self[q], ascending; pairs beyond the band listed at w + 1, smallest ids first.
//
// The store is projected once (k_po_project of ed_po.hip) and stays resident with a 256-byte profile per trace.
// k_po_knn_profile: one wave per trace. The row of projected offsets goes to LDS as
// 32-bit starts relative to the trace; lenfold[b] sums the lengths of the entities g = b (mod 32); every element of
// the flat projected range finds its entity by binary search in the starts, takes prev from its left neighbour (the
// constant at a segment start) and counts the bucket mix(mix(prev + g) ^ cur) >> 57 in an LDS counter; the 128
// counters are written saturated at 255, four to a word.
// k_po_knn (K11b): work item = (query, block of 64 stored traces, part p of P), taken by persistent waves from a
// counter (a stride deal leaves a wave whose items ran long holding the launch's end; K8's note on idle slots). A
// search with fewer blocks than four per wave cuts every block's survivors into P <= 64 parts -- the s-th survivor
// goes to part s mod P, every part repeats the block's filter (16 KiB from L2) and part 0 counts it -- so that one
// query against 4,096 stored traces is 3,072 items of at most two DPs and not 64 items of 64.
//   filter  a lane per candidate: the query's profile is uniform, the lane reads its candidate's 256 bytes;
//           LB_len = sum_b |lenfold_q[b] - lenfold_c[b]|, LB_gram = ceil(sum_h |gram_q[h] - gram_c[h]| / 4) by
//           v_sad_u8; max(LB_len, LB_gram) > w settles the pair at w + 1. One ballot gives the survivors.
//   DP      the wave per surviving pair, distance only. The two rows of projected offsets 64 entities at a time:
//           first the exact sum of ||q|g| - |c|g|| (> w: beyond, no DP), then for every entity where either side is
//           not empty, ascending, the cell-form row step without history (ed_align_dev.h: 2w + 1 cells blocked over
//           the lanes, C in {1, 2, 3}, the DPP min-scan closure, q|g and the window of c|g staged in LDS per 64
//           rows). Entity g runs against the budget r = w - (the sum so far): a row without a cell <= r, or a
//           result > r, ends the pair at w + 1 (Lev_g > r => the sum > w: exact).
//   lists   in-band results go into the query's list by knn_insert; k_po_knn_fill completes the lists with
//           (w + 1, the smallest ids not listed and not q_self).
// Counters, striped as the bit-parallel search keeps them: 0 pairs settled by the filter, 1 pairs settled by the
// exact length sum, 2 pairs that ran a DP, 3 pairs in band. Plain vector stores and atomics on the lists only.
//
// Bands 65 .. 1,024 (the nmz_po_knn_wide_* entry points, at this file's end): the same plan, validators, batcher and
// enqueue; pk_enqueue launches K11w (k_po_knn_wide, ed_po_knn_wide.hip) in K11b's place when the plan's band is
// above 64. ed_po_knn.h holds what the two kernels share: the argument block, the filter, the counters' layout.
#include <algorithm>
#include <string>
#include <vector>

#include "ed_align_dev.h"
#include "ed_knn_dev.h"
#include "ed_plan.h"
#include "ed_po_knn.h"
#include "nmz_common.h"
#include "nmz_internal.h"

namespace nmz {

constexpr uint32_t PK_WAVES_PER_CU = 12;         // persistent waves of k_po_knn: 3 per SIMD (144 .. 154 VGPRs)
constexpr uint32_t PK_PROF_BLOCKS_PER_CU = 16;   // k_po_knn_profile: one wave per workgroup
constexpr uint64_t PK_GRAM_START = 0x9E3779B97F4A7C15ull;
static_assert(NMZ_PO_KNN_MAX_BAND == 64 && NMZ_PO_KNN_MAX_K == 64, "three cells per lane cover 2 * 64 + 1");

__host__ __device__ inline uint64_t pk_mix(uint64_t x) {
    x ^= x >> 30;
    x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27;
    x *= 0x94D049BB133111EBull;
    x ^= x >> 31;
    return x;
}
__host__ __device__ inline uint32_t pk_bucket(uint32_t g, uint64_t prev, uint64_t cur) {
    return (uint32_t)(pk_mix(pk_mix(prev + g) ^ cur) >> 57);
}

// ---- the guard of the device form: offsets that cannot leave the plan's query scratch ----
// safe[i] = min(max(q_off[0 .. i]), cap): non-decreasing and <= cap whatever the caller passed; *over = 1 when the
// caller's offsets do not start at 0, decrease or exceed cap (the search then writes nothing: every list stays empty).
__global__ __launch_bounds__(64) void k_po_knn_qoff(const uint64_t *__restrict__ q_off, uint32_t n_queries, uint64_t cap,
                                                    uint64_t *__restrict__ safe, uint32_t *__restrict__ over) {
    const uint32_t lane = threadIdx.x;
    uint64_t run = 0;
    bool bad = false;
    for (uint64_t i0 = 0; i0 <= n_queries; i0 += 64) {
        const uint64_t i = i0 + lane;
        const uint64_t raw = i <= n_queries ? q_off[i] : 0;
        uint64_t v = raw;
#pragma unroll
        for (uint32_t o = 1; o < 64; o <<= 1) {
            const uint64_t u = __shfl_up(v, o, 64);
            v = lane >= o && u > v ? u : v;
        }
        v = v > run ? v : run;
        bad = bad || (i <= n_queries && (raw < v || raw > cap || (i == 0 && raw != 0)));
        if (i <= n_queries) safe[i] = v < cap ? v : cap;
        run = __shfl(v, 63, 64);
    }
    const uint64_t any = __ballot(bad);
    if (lane == 0) *over = any ? 1u : 0u;
}

// ---- K11a ----
__global__ __launch_bounds__(64) void k_po_knn_profile(const uint64_t *__restrict__ poff, const uint64_t *__restrict__ psym,
                                                       uint32_t n_traces, uint32_t G, uint32_t *__restrict__ prof) {
    extern __shared__ uint32_t pk_lds[];  // rel[G + 1], then cnt[128]
    uint32_t *rel = pk_lds, *cnt = pk_lds + G + 1;
    const uint32_t lane = threadIdx.x;
    for (uint64_t t = blockIdx.x; t < n_traces; t += gridDim.x) {
        const uint64_t *row = poff + t * G;
        const uint64_t base = row[0];
        __syncthreads();  // the previous trace's reads of rel and cnt
        for (uint32_t i = lane; i <= G; i += 64) rel[i] = (uint32_t)(row[i] - base);
        cnt[lane] = 0;
        cnt[lane + 64] = 0;
        __syncthreads();
        uint32_t lf = 0;  // entities lane, lane + 64, ...: all = lane (mod 32)
        for (uint32_t e = lane; e < G; e += 64) lf += rel[e + 1] - rel[e];
        lf += __shfl_xor(lf, 32, 64);
        const uint32_t total = rel[G];
        for (uint32_t q = lane; q < total; q += 64) {
            // the entity of element q: the last e with rel[e] <= q (rel[0] = 0; its segment is not empty)
            uint32_t lo = 0, n = G;
            while (n > 1) {
                const uint32_t h = n >> 1;
                lo = rel[lo + h] <= q ? lo + h : lo;
                n -= h;
            }
            const uint64_t cur = psym[base + q];
            const uint64_t prev = q == rel[lo] ? PK_GRAM_START : psym[base + q - 1];
            atomicAdd(&cnt[pk_bucket(lo, prev, cur)], 1u);
        }
        __syncthreads();
        uint32_t *out = prof + t * PK_PROF_WORDS;
        if (lane < 32) {
            out[lane] = lf;
            uint32_t wd = 0;
#pragma unroll
            for (uint32_t b = 0; b < 4; ++b) wd |= min(cnt[4 * lane + b], 255u) << (8 * b);
            out[32 + lane] = wd;
        }
    }
}

// ---- K11b ----
// PkArgs, pk_wave_sum, pk_lane64 and the filter (pk_filter_passes): ed_po_knn.h, shared with K11w

// Lev(a, b) when it is <= r, anything > r otherwise; |n - m| <= r <= w. The band's cells are laid out for w.
template <int C>
__device__ __forceinline__ uint32_t pk_lev(const uint64_t *__restrict__ a, int64_t n, const uint64_t *__restrict__ b,
                                           int64_t m, int32_t w, int32_t r, uint64_t *s_a, uint64_t *s_b,
                                           uint32_t lane) {
    const int32_t d0 = (int32_t)lane * C;  // this lane's first cell
    int32_t prev[C];
    AlignNoMoves distance_only;
    align_row0<C>(prev, d0, w, m);
    for (int64_t i0 = 0; i0 < n; i0 += ALIGN_ROWS) {
        const int32_t rows = (int32_t)min((int64_t)ALIGN_ROWS, n - i0);
        align_stage<int, 64>(s_a, s_b, a, n, b, m, i0, w, lane);
        for (int32_t rr = 1; rr <= rows; ++rr) {
            const uint64_t ai = s_a[rr - 1];
            const int32_t nxt = align_dpp<DPP_WAVE_SHL1>(ALIGN_INF, prev[0]);  // the next lane's first cell
            int32_t t[C], lp[C];
            bool valid[C];
            align_row_candidates<C>(prev, nxt, ai, s_b, rr, d0, w, m, i0 + rr, t, valid, lp, distance_only);
            const int32_t excl = align_dpp<DPP_WAVE_SHR1>(ALIGN_INF, align_scan_min(lp[C - 1]));  // lanes below
            const bool live = align_row_close<C>(prev, valid, lp, excl, d0, r, distance_only);
            if (__ballot(live) == 0) return (uint32_t)r + 1;  // the row's minimum has passed the budget
        }
    }
    const int32_t df = (int32_t)(m - n) + w;  // in [0, 2 w]
    return (uint32_t)min(__builtin_amdgcn_readlane(align_final_cell<C>(prev, df), df / C), r + 1);
}

template <int C>
__global__ __launch_bounds__(64) void k_po_knn(const PkArgs g) {
    __shared__ uint64_t s_a[ALIGN_ROWS];
    __shared__ uint64_t s_b[ALIGN_ROWS + 2 * NMZ_PO_KNN_MAX_BAND];
    if (*g.over) return;
    const uint32_t lane = threadIdx.x;
    const uint32_t w = g.w, G = g.G;
    uint64_t n_filter = 0, n_len = 0, n_dp = 0, n_in = 0;  // wave-uniform
    for (;;) {
        unsigned long long item = 0;
        if (lane == 0) item = atomicAdd(g.next, 1ull);
        item = pk_lane64(item, 0);
        if (item >= g.n_items) break;
        const uint64_t blk = item / g.parts;
        const uint32_t part = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(item - blk * g.parts));
        const uint32_t q = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(blk / g.NB));
        const uint32_t cb = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(blk - (uint64_t)q * g.NB));
        const uint32_t self = g.q_self ? g.q_self[q] : NMZ_NONE;
        const uint32_t cand = cb * 64 + lane;
        const bool valid = cand < g.N && cand != self;
        bool survive = valid;
        if (!g.no_filter) {
            // ---- the filter: a lane per candidate
            const uint32_t *__restrict__ qp = g.q_prof + (uint64_t)q * PK_PROF_WORDS;  // uniform
            const uint4 *__restrict__ cp = (const uint4 *)(g.prof + (uint64_t)(valid ? cand : 0) * PK_PROF_WORDS);
            const bool passes = pk_filter_passes(qp, cp, w);  // every lane: no branch round the loads
            survive = valid && passes;
        }
        uint64_t todo = __ballot(survive);
        if (part == 0) n_filter += (uint32_t)__popcll(__ballot(valid)) - (uint32_t)__popcll(todo);
        uint32_t nth = 0;  // of the block's survivors
        const uint64_t *__restrict__ qrow = g.q_poff + (uint64_t)q * G;
        // ---- the DP: the wave per surviving pair
        while (todo) {  // wave-uniform
            const uint32_t bit = (uint32_t)__builtin_amdgcn_readfirstlane(__ffsll((unsigned long long)todo) - 1);
            todo &= todo - 1;
            if (nth++ % g.parts != part) continue;  // another part's pair
            const uint32_t c = cb * 64 + bit;
            const uint64_t *__restrict__ crow = g.poff + (uint64_t)c * G;
            // the exact sum of the entities' length differences
            uint32_t lsum = 0;
            for (uint32_t g0 = 0; g0 < G && lsum <= w; g0 += 64) {
                const uint32_t e = g0 + lane;
                uint32_t diff = 0;
                if (e < G) {
                    const uint64_t la = qrow[e + 1] - qrow[e], lb = crow[e + 1] - crow[e];
                    diff = (uint32_t)min(la > lb ? la - lb : lb - la, (uint64_t)w + 1);
                }
                lsum += pk_wave_sum(diff);  // <= 64 * 65 per chunk, <= 16 chunks
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
                while (ents) {  // wave-uniform, ascending entity
                    const int src = __builtin_amdgcn_readfirstlane(__ffsll((unsigned long long)ents) - 1);
                    ents &= ents - 1;
                    const uint64_t a0 = pk_lane64(qlo, src), a1 = pk_lane64(qhi, src);
                    const uint64_t b0 = pk_lane64(clo, src), b1 = pk_lane64(chi, src);
                    const int64_t n = (int64_t)(a1 - a0), m = (int64_t)(b1 - b0);
                    const int32_t r = (int32_t)(w - sum);
                    if ((n > m ? n - m : m - n) > (int64_t)r) {
                        beyond = true;
                        break;
                    }
                    const uint32_t d = pk_lev<C>(g.q_psym + a0, n, g.psym + b0, m, (int32_t)w, r, s_a, s_b, lane);
                    if (d > (uint32_t)r) {
                        beyond = true;
                        break;
                    }
                    sum += d;
                }
            }
            if (!beyond) {
                ++n_in;
                if (lane == 0) knn_insert(g.knn + (uint64_t)q * g.k, g.k, ((uint64_t)sum << 32) | c);
            }
        }
    }
    if (lane < PK_NCOUNTERS) {
        const uint64_t v = lane == 0 ? n_filter : (lane == 1 ? n_len : (lane == 2 ? n_dp : n_in));
        if (v) atomicAdd((unsigned long long *)&g.counters[(blockIdx.x % ED_CNT_STRIPES) * ED_CNT_LINE + lane],
                         (unsigned long long)v);
    }
}

// a search's start: the lists, the counters and the item counter in one launch
__global__ void k_po_knn_init(uint64_t *knn, uint64_t n, uint64_t *counters, unsigned long long *next) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) knn[i] = UINT64_MAX;
    if (i < ED_CNT_WORDS) counters[i] = 0;
    if (i == 0) *next = 0;
}

// k_knn_fill (ed.hip) with the id to skip taken per list: list i takes (fill_d, j) for the smallest ids j < n_cand
// that are not listed and not q_self[i], in increasing j, until it holds k keys (UINT64_MAX where fewer exist)
__global__ void k_po_knn_fill(uint64_t *knn, uint32_t n_lists, uint32_t k, uint32_t n_cand, uint32_t fill_d,
                              const uint32_t *__restrict__ q_self, const uint32_t *__restrict__ over) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_lists || *over) return;
    const uint32_t self = q_self ? q_self[i] : NMZ_NONE;
    uint64_t *L = knn + (uint64_t)i * k;
    uint32_t c = 0;
    while (c < k && L[c] != UINT64_MAX && (uint32_t)(L[c] >> 32) < fill_d) ++c;
    uint32_t j = 0;
    for (uint32_t s = c; s < k; ++s) {
        for (;; ++j) {
            if (j >= n_cand) break;
            if (j == self) continue;
            bool listed = false;
            for (uint32_t t = 0; t < c; ++t) listed |= (uint32_t)L[t] == j;
            if (!listed) break;
        }
        L[s] = j < n_cand ? (((uint64_t)fill_d << 32) | j) : UINT64_MAX;
        ++j;
    }
}

// ---- the limits, no device ----
static int pk_band(uint32_t band) {
    NMZ_CHECK(band <= NMZ_PO_KNN_MAX_BAND, "band " + std::to_string(band) +
                                               " exceeds NMZ_PO_KNN_MAX_BAND (64): the PO search over wider bands is "
                                               "not built yet");
    return NMZ_OK;
}

// the same for the wide entry points (K11w: 65 .. 1,024; a band <= 64 runs K11b)
static int pkw_band(uint32_t band) {
    NMZ_CHECK(band <= NMZ_PO_KNN_WIDE_MAX_BAND, "band " + std::to_string(band) +
                                                    " exceeds NMZ_PO_KNN_WIDE_MAX_BAND (1024): the PO search over "
                                                    "wider bands is not built yet");
    return NMZ_OK;
}
typedef int (*PkBandCheck)(uint32_t band);

static int pk_k(uint32_t k) {
    NMZ_CHECK(k >= 1 && k <= NMZ_PO_KNN_MAX_K, "k " + std::to_string(k) + " must be 1 .. NMZ_PO_KNN_MAX_K (64)");
    return NMZ_OK;
}

static int pk_entities(uint32_t G) {
    NMZ_CHECK(G >= 1 && G <= NMZ_PO_MAX_ENTITIES,
              "n_entities " + std::to_string(G) + " must be 1 .. NMZ_PO_MAX_ENTITIES (1024)");
    return NMZ_OK;
}

static int pk_count(const char *what, uint64_t n, uint32_t G) {
    NMZ_CHECK(n * G < (1ull << 31) - 1, std::string(what) + " * n_entities = " + std::to_string(n) + " * " +
                                            std::to_string(G) +
                                            " must stay below 2^31 - 1: the projected traces are indexed with 32 bits");
    return NMZ_OK;
}

// one CSR with its entities: `what` is "store" or "query", `count` the name of n in the messages
static int pk_csr(const char *what, const char *count, const uint64_t *off, const uint64_t *sym, const uint32_t *ent,
                  uint32_t n, uint32_t G) {
    const std::string W(what);
    NMZ_TRY(pk_count(count, n, G));
    if (n == 0) return NMZ_OK;
    NMZ_CHECK(off != nullptr, W + " offsets are NULL");
    NMZ_CHECK(off[0] == 0, W + " offsets must start at 0");
    for (uint32_t t = 0; t < n; ++t) {
        NMZ_CHECK(off[t] <= off[t + 1], W + " offsets must be non-decreasing (trace " + std::to_string(t) + ")");
        NMZ_CHECK(off[t + 1] - off[t] < 0xFFFFFFFFull, W + " trace " + std::to_string(t) + " has " +
                                                           std::to_string(off[t + 1] - off[t]) +
                                                           " elements: at most 2^32 - 2");
    }
    const uint64_t total = off[n];
    NMZ_CHECK(total == 0 || sym, W + " sym is NULL");
    NMZ_CHECK(total == 0 || ent, W + " entity is NULL");
    for (uint64_t i = 0; i < total; ++i)
        NMZ_CHECK(ent[i] < G || ent[i] == NMZ_NONE,
                  W + " element " + std::to_string(i) + " has entity id " + std::to_string(ent[i]) +
                      ": ids are < n_entities (" + std::to_string(G) + ") or NMZ_NONE");
    return NMZ_OK;
}

static int pk_self(const uint32_t *q_self, uint32_t n_queries, uint32_t n_traces) {
    if (!q_self) return NMZ_OK;
    for (uint32_t i = 0; i < n_queries; ++i)
        NMZ_CHECK(q_self[i] < n_traces || q_self[i] == NMZ_NONE,
                  "q_self[" + std::to_string(i) + "] = " + std::to_string(q_self[i]) + ": a store index < n_traces (" +
                      std::to_string(n_traces) + ") or NMZ_NONE");
    return NMZ_OK;
}

}  // namespace nmz

struct nmz_po_knn_plan {
    nmz_ctx *ctx = nullptr;
    uint32_t band = 0, G = 0, N = 0, opts = 0;
    uint64_t max_queries = 0, max_query_elems = 0;
    nmz::DevBuf store;  // poff, psym, prof: resident
    uint64_t *poff = nullptr, *psym = nullptr;
    uint32_t *prof = nullptr;
    nmz::DevBuf query;  // the query-side scratch of the _dev form
    uint64_t *q_safe = nullptr, *q_poff = nullptr, *q_psym = nullptr, *counters = nullptr;
    uint32_t *q_psrc = nullptr, *q_prof = nullptr, *over = nullptr;
    unsigned long long *next = nullptr;
    uint64_t resident_bytes = 0;
    uint32_t blocks = 0, waves = 0;  // of the latest k_po_knn launch
    nmz::PlanFence fence;  // the query scratch serves one stream at a time
};

namespace nmz {

static void pk_plan_destroy_locked(nmz_po_knn_plan *p) {
    p->fence.destroy();
    p->store.release();
    p->query.release();
    delete p;
}

static int pk_profile_enqueue(nmz_ctx *ctx, hipStream_t st, const uint64_t *d_poff, const uint64_t *d_psym, uint32_t n,
                              uint32_t G, uint32_t *d_prof) {
    if (n == 0) return NMZ_OK;
    const unsigned blocks = (unsigned)std::min<uint64_t>(n, (uint64_t)std::max(ctx->n_cu, 1) * PK_PROF_BLOCKS_PER_CU);
    KernelTimer kt(ctx, st, "po_knn_profile");
    hipLaunchKernelGGL(k_po_knn_profile, dim3(blocks), dim3(64), (size_t)(G + 1 + 128) * sizeof(uint32_t), st, d_poff,
                       d_psym, n, G, d_prof);
    if (hipGetLastError() != hipSuccess) return fail(NMZ_EHIP, "k_po_knn_profile launch failed");
    return NMZ_OK;
}

// the plan's own limits, no device; known = the opts bits of the entry point
static int pk_plan_shape(PkBandCheck band_ok, uint32_t known, uint32_t band, uint32_t G, uint64_t max_queries,
                         uint32_t opts) {
    NMZ_TRY(band_ok(band));
    NMZ_TRY(pk_entities(G));
    NMZ_CHECK(max_queries >= 1, "max_queries is 0");
    NMZ_TRY(pk_count("max_queries", max_queries, G));
    NMZ_CHECK((opts & ~known) == 0, "opts " + std::to_string(opts) + ": unknown bits");
    return NMZ_OK;
}
constexpr uint32_t PK_OPTS = NMZ_PO_KNN_OPT_NO_FILTER | NMZ_PO_KNN_OPT_WHOLE_BLOCKS;
constexpr uint32_t PKW_OPTS = PK_OPTS | NMZ_PO_KNN_OPT_FULL_BAND;

// upload, project and profile the store, size the query scratch; the caller holds ctx and has validated
static int pk_plan_create_locked(nmz_ctx *ctx, const uint64_t *off, const uint64_t *sym, const uint32_t *entity,
                                 uint32_t N, uint32_t G, uint32_t band, uint64_t max_queries, uint64_t max_query_elems,
                                 uint32_t opts, nmz_po_knn_plan **out) {
    auto *p = new nmz_po_knn_plan();
    p->ctx = ctx;
    p->band = band;
    p->G = G;
    p->N = N;
    p->opts = opts;
    p->max_queries = max_queries;
    p->max_query_elems = max_query_elems;
    p->store.pool = &ctx->pool;
    p->query.pool = &ctx->pool;
    const uint64_t total = N ? off[N] : 0;
    hipStream_t st = ctx->stream;
    DevBuf tmp;  // the unprojected store and psrc: not needed once the profiles are made
    tmp.pool = &ctx->pool;
    int rc = NMZ_OK;
    auto build = [&]() -> int {
        ScratchLayout ls, lq, lt;
        ls.add(&p->poff, (size_t)N * G + 1).add(&p->psym, total + 1).add(&p->prof, (size_t)N * PK_PROF_WORDS + 1);
        NMZ_TRY(ls.bind(p->store));
        lq.add(&p->q_safe, max_queries + 1).add(&p->q_poff, (size_t)max_queries * G + 1);
        lq.add(&p->q_psym, max_query_elems + 1).add(&p->q_psrc, max_query_elems + 1);
        lq.add(&p->q_prof, (size_t)max_queries * PK_PROF_WORDS).add(&p->counters, ED_CNT_WORDS).add(&p->next, 1);
        lq.add(&p->over, 1);
        NMZ_TRY(lq.bind(p->query));
        p->resident_bytes = ls.bytes() + lq.bytes();
        NMZ_TRY(p->fence.create("po knn plan"));
        NMZ_HIP(hipMemsetAsync(p->counters, 0, ED_CNT_WORDS * sizeof(uint64_t), st));
        NMZ_HIP(hipMemsetAsync(p->over, 0, sizeof(uint32_t), st));
        uint64_t *d_off, *d_sym;
        uint32_t *d_ent, *d_psrc;
        lt.add(&d_off, (size_t)N + 1).add(&d_sym, total + 1).add(&d_ent, total + 1).add(&d_psrc, total + 1);
        NMZ_TRY(lt.bind(tmp));
        if (N) {
            NMZ_TRY(upload_csr(d_off, d_sym, off, sym, N, st));
            NMZ_TRY(copy_h2d(d_ent, entity, total, st));
        }
        NMZ_TRY(po_project_enqueue(ctx, st, d_off, d_sym, d_ent, N, G, p->poff, p->psym, d_psrc));
        NMZ_TRY(pk_profile_enqueue(ctx, st, p->poff, p->psym, N, G, p->prof));
        NMZ_HIP(hipStreamSynchronize(st));
        return NMZ_OK;
    };
    rc = build();
    if (rc != NMZ_OK) (void)hipStreamSynchronize(st);
    tmp.release();
    if (rc != NMZ_OK) {
        pk_plan_destroy_locked(p);
        return rc;
    }
    *out = p;
    return NMZ_OK;
}

// the guard, the queries' projection and profiles, K11b and the fill on `st`, nothing else; the caller holds ctx
static int pk_enqueue(nmz_po_knn_plan *p, hipStream_t st, const uint64_t *d_q_off, const uint64_t *d_q_sym,
                      const uint32_t *d_q_ent, const uint32_t *d_q_self, uint32_t n_queries, uint32_t k,
                      uint64_t *d_keys) {
    NMZ_TRY(pk_k(k));
    NMZ_CHECK(n_queries <= p->max_queries, "n_queries " + std::to_string(n_queries) +
                                               " exceeds the plan's max_queries (" + std::to_string(p->max_queries) +
                                               "); max_query_elems is " + std::to_string(p->max_query_elems));
    if (n_queries == 0) return NMZ_OK;
    NMZ_CHECK(d_q_off && d_q_sym && d_q_ent && d_keys, "d_q_off, d_q_sym, d_q_entity or d_knn_keys is NULL");
    nmz_ctx *ctx = p->ctx;
    NMZ_TRY(p->fence.enter(st));
    const uint32_t G = p->G, N = p->N;
    hipLaunchKernelGGL(k_po_knn_qoff, dim3(1), dim3(64), 0, st, d_q_off, n_queries, p->max_query_elems, p->q_safe,
                       p->over);
    if (hipGetLastError() != hipSuccess) return fail(NMZ_EHIP, "k_po_knn_qoff launch failed");
    int rc = po_project_enqueue(ctx, st, p->q_safe, d_q_sym, d_q_ent, n_queries, G, p->q_poff, p->q_psym, p->q_psrc);
    if (rc == NMZ_OK) rc = pk_profile_enqueue(ctx, st, p->q_poff, p->q_psym, n_queries, G, p->q_prof);
    const uint64_t nk = (uint64_t)n_queries * k;
    if (rc == NMZ_OK) {
        const uint64_t nt = std::max<uint64_t>(nk, ED_CNT_WORDS);
        hipLaunchKernelGGL(k_po_knn_init, dim3(ceil_div(nt, 256)), dim3(256), 0, st, d_keys, nk, p->counters, p->next);
        if (hipGetLastError() != hipSuccess) rc = fail(NMZ_EHIP, "k_po_knn_init launch failed");
    }
    if (rc == NMZ_OK && N > 0) {
        PkArgs a{};
        a.poff = p->poff, a.psym = p->psym, a.prof = p->prof;
        a.q_poff = p->q_poff, a.q_psym = p->q_psym, a.q_prof = p->q_prof, a.q_self = d_q_self;
        a.N = N, a.G = G, a.k = k, a.w = p->band;
        a.no_filter = (p->opts & NMZ_PO_KNN_OPT_NO_FILTER) ? 1u : 0u;
        a.full_band = (p->opts & NMZ_PO_KNN_OPT_FULL_BAND) ? 1u : 0u;
        a.NB = (N + 63) / 64;
        const bool wide = p->band > NMZ_PO_KNN_MAX_BAND;  // K11w: the persistent unit is a workgroup of four waves
        const uint64_t n_blocks = (uint64_t)n_queries * a.NB;
        const uint64_t cap = wide ? pkw_resident(ctx, p->band) : (uint64_t)std::max(ctx->n_cu, 1) * PK_WAVES_PER_CU;
        a.parts = 1;  // fewer than PK_ITEMS_PER_WAVE blocks per wave: the blocks' survivors in parts
        if (!(p->opts & NMZ_PO_KNN_OPT_WHOLE_BLOCKS))
            a.parts = (uint32_t)std::min<uint64_t>(64, (PK_ITEMS_PER_WAVE * cap + n_blocks - 1) / n_blocks);
        a.n_items = n_blocks * a.parts;
        a.knn = d_keys, a.counters = p->counters, a.next = p->next, a.over = p->over;
        const unsigned blocks = (unsigned)std::min<uint64_t>(a.n_items, cap);
        p->blocks = blocks;
        p->waves = wide ? blocks * AW_WAVES : blocks;  // K11b: the workgroup is the wave
        if (wide) {
            rc = pkw_launch(ctx, st, a, blocks);
        } else {
            KernelTimer kt(ctx, st, "po_knn");
            switch (align_cells(p->band)) {
                case 1: hipLaunchKernelGGL(k_po_knn<1>, dim3(blocks), dim3(64), 0, st, a); break;
                case 2: hipLaunchKernelGGL(k_po_knn<2>, dim3(blocks), dim3(64), 0, st, a); break;
                default: hipLaunchKernelGGL(k_po_knn<3>, dim3(blocks), dim3(64), 0, st, a); break;
            }
            if (hipGetLastError() != hipSuccess) rc = fail(NMZ_EHIP, "k_po_knn launch failed");
        }
        if (rc == NMZ_OK) {
            KernelTimer kt(ctx, st, "po_knn_fill");
            hipLaunchKernelGGL(k_po_knn_fill, dim3(ceil_div(n_queries, 256)), dim3(256), 0, st, d_keys, n_queries, k, N,
                               p->band + 1, d_q_self, p->over);
            if (hipGetLastError() != hipSuccess) rc = fail(NMZ_EHIP, "k_po_knn_fill launch failed");
        }
    }
    NMZ_TRY(p->fence.leave(st));
    return rc;
}

// every limit of the queries of a host form against a store of n_traces traces, no device
static int pk_validate_queries(const uint64_t *q_off, const uint64_t *q_sym, const uint32_t *q_entity,
                               const uint32_t *q_self, uint32_t n_queries, uint32_t n_traces, uint32_t G,
                               const uint32_t *knn_id, const uint32_t *knn_dist) {
    NMZ_TRY(pk_csr("query", "n_queries", q_off, q_sym, q_entity, n_queries, G));
    NMZ_TRY(pk_self(q_self, n_queries, n_traces));
    NMZ_CHECK(n_queries == 0 || (knn_id && knn_dist), "knn_id or knn_dist is NULL");
    return NMZ_OK;
}

// the host form's body behind its checks: batches by the plan's capacity on the context's stream, one drain
static int pk_query_locked(nmz_po_knn_plan *p, HostCall &call, const std::vector<uint64_t> &boff,
                           const std::vector<uint32_t> &bstart, const uint64_t *q_off, const uint64_t *q_sym,
                           const uint32_t *q_entity, const uint32_t *q_self, uint32_t n_queries, uint32_t k,
                           uint32_t *knn_id, uint32_t *knn_dist) {
    hipStream_t st = call.st;
    const uint64_t total = q_off[n_queries], nk = (uint64_t)n_queries * k;
    uint64_t *d_boff, *d_sym, *d_keys;
    uint32_t *d_ent, *d_self, *d_id, *d_ds;
    ScratchLayout lay;
    lay.add(&d_boff, boff.size()).add(&d_sym, total + 1).add(&d_ent, total + 1).add(&d_self, n_queries);
    lay.add(&d_keys, nk).add(&d_id, nk).add(&d_ds, nk);
    NMZ_TRY(lay.bind(call.work));
    NMZ_TRY(copy_h2d(d_boff, boff.data(), boff.size(), st));
    NMZ_TRY(copy_h2d(d_sym, q_sym, total, st));
    NMZ_TRY(copy_h2d(d_ent, q_entity, total, st));
    if (q_self) NMZ_TRY(copy_h2d(d_self, q_self, n_queries, st));
    for (size_t b = 0; b + 1 < bstart.size(); ++b) {
        const uint32_t q0 = bstart[b], nb = bstart[b + 1] - q0;
        NMZ_TRY(pk_enqueue(p, st, d_boff + q0 + b, d_sym + q_off[q0], d_ent + q_off[q0], q_self ? d_self + q0 : nullptr,
                           nb, k, d_keys + (uint64_t)q0 * k));
    }
    return knn_final_to_host(call, d_keys, nk, d_id, d_ds, knn_id, knn_dist);
}

// the batches of a host call: bstart[b] = the first query of batch b (and n_queries at the end); boff = the batches'
// offsets, each rebased to 0, nb + 1 words per batch one after the other
static int pk_batches(const uint64_t *q_off, uint32_t n_queries, uint64_t max_queries, uint64_t max_elems,
                      std::vector<uint64_t> &boff, std::vector<uint32_t> &bstart) {
    uint32_t q0 = 0;
    while (q0 < n_queries) {
        uint32_t q1 = q0;
        while (q1 < n_queries && q1 - q0 < max_queries && q_off[q1 + 1] - q_off[q0] <= max_elems) ++q1;
        NMZ_CHECK(q1 > q0, "query " + std::to_string(q0) + " has " + std::to_string(q_off[q0 + 1] - q_off[q0]) +
                               " elements: more than the plan's max_query_elems (" + std::to_string(max_elems) + ")");
        bstart.push_back(q0);
        for (uint32_t q = q0; q <= q1; ++q) boff.push_back(q_off[q] - q_off[q0]);
        q0 = q1;
    }
    bstart.push_back(n_queries);
    return NMZ_OK;
}

// the body of the two plan creates: band_ok and `known` (the opts bits) are the entry point's
static int pk_plan_create_call(PkBandCheck band_ok, uint32_t known, nmz_ctx *ctx, const uint64_t *off,
                               const uint64_t *sym, const uint32_t *entity, uint32_t n_traces, uint32_t n_entities,
                               uint32_t band, uint64_t max_queries, uint64_t max_query_elems, uint32_t opts,
                               nmz_po_knn_plan **out) {
    NMZ_CHECK(out != nullptr, "out is NULL");
    *out = nullptr;
    // the arguments first: they are checked without a device
    NMZ_TRY(pk_plan_shape(band_ok, known, band, n_entities, max_queries, opts));
    NMZ_TRY(pk_csr("store", "n_traces", off, sym, entity, n_traces, n_entities));
    NMZ_CHECK(ctx != nullptr, "ctx is NULL");
    CtxGuard g(ctx);
    NMZ_TRY(g.rc);
    return pk_plan_create_locked(ctx, off, sym, entity, n_traces, n_entities, band, max_queries, max_query_elems, opts,
                                 out);
}

// the body of the two one-shot forms
static int pk_one_shot(PkBandCheck band_ok, nmz_ctx *ctx, const uint64_t *off, const uint64_t *sym,
                       const uint32_t *entity, uint32_t n_traces, uint32_t n_entities, const uint64_t *q_off,
                       const uint64_t *q_sym, const uint32_t *q_entity, const uint32_t *q_self, uint32_t n_queries,
                       uint32_t band, uint32_t k, uint32_t *knn_id, uint32_t *knn_dist) {
    // the arguments first: they are checked without a device
    NMZ_TRY(band_ok(band));
    NMZ_TRY(pk_k(k));
    NMZ_TRY(pk_entities(n_entities));
    NMZ_TRY(pk_csr("store", "n_traces", off, sym, entity, n_traces, n_entities));
    NMZ_TRY(pk_validate_queries(q_off, q_sym, q_entity, q_self, n_queries, n_traces, n_entities, knn_id, knn_dist));
    if (n_queries == 0) return NMZ_OK;  // nothing to write: no device either
    if (n_traces == 0) {                // nothing to find: no device either
        std::fill(knn_id, knn_id + (size_t)n_queries * k, NMZ_NONE);
        std::fill(knn_dist, knn_dist + (size_t)n_queries * k, NMZ_NONE);
        return NMZ_OK;
    }
    std::vector<uint64_t> boff;
    std::vector<uint32_t> bstart;
    NMZ_TRY(pk_batches(q_off, n_queries, n_queries, q_off[n_queries], boff, bstart));
    NMZ_CHECK(ctx != nullptr, "ctx is NULL");
    CtxGuard g(ctx);
    NMZ_TRY(g.rc);
    HostCall call(ctx);
    nmz_po_knn_plan *plan = nullptr;
    NMZ_TRY(pk_plan_create_locked(ctx, off, sym, entity, n_traces, n_entities, band, n_queries, q_off[n_queries], 0,
                                  &plan));
    call.own_plan<pk_plan_destroy_locked>(plan);
    return pk_query_locked(plan, call, boff, bstart, q_off, q_sym, q_entity, q_self, n_queries, k, knn_id, knn_dist);
}

// the first n words of the latest search's counters, the stripes summed
static int pk_counters(nmz_po_knn_plan *plan, uint64_t *out, uint32_t n, void *stream) {
    NMZ_CHECK(plan != nullptr, "plan is NULL");
    NMZ_CHECK(out != nullptr, "out is NULL");
    CtxGuard g(plan->ctx);
    NMZ_TRY(g.rc);
    hipStream_t st = stream ? (hipStream_t)stream : plan->ctx->stream;
    std::vector<uint64_t> h(ED_CNT_WORDS);
    uint32_t over = 0;
    NMZ_TRY(copy_d2h(h.data(), plan->counters, ED_CNT_WORDS, st));
    NMZ_TRY(copy_d2h(&over, plan->over, 1, st));
    NMZ_HIP(hipStreamSynchronize(st));
    for (uint32_t i = 0; i < n; ++i) out[i] = 0;
    for (uint32_t s = 0; s < ED_CNT_STRIPES; ++s)
        for (uint32_t i = 0; i < n; ++i) out[i] += h[s * ED_CNT_LINE + i];
    NMZ_CHECK(!over, "the latest search's query offsets did not start at 0, decreased or exceeded the plan's "
                     "max_query_elems (" + std::to_string(plan->max_query_elems) + "): it wrote no list");
    return NMZ_OK;
}

}  // namespace nmz

using namespace nmz;

extern "C" {

// The two lower bounds of one pair on the calling thread, by the definition (historystorage.go:50-51,
// naive.go:235-257, visualize.go:62-136): plain vectors per entity, one pass, nothing shared with K11.
int nmz_po_knn_bound_host(const uint64_t *a, const uint32_t *ea, uint64_t n, const uint64_t *b, const uint32_t *eb,
                          uint64_t m, uint32_t n_entities, uint32_t *lb_len, uint32_t *lb_gram) {
    NMZ_CHECK(n < 0xFFFFFFFFull, "a has " + std::to_string(n) + " elements: at most 2^32 - 2");
    NMZ_CHECK(m < 0xFFFFFFFFull, "b has " + std::to_string(m) + " elements: at most 2^32 - 2");
    NMZ_CHECK((n == 0 || (a && ea)) && (m == 0 || (b && eb)), "a, b or an entity array is NULL");
    NMZ_CHECK(lb_len && lb_gram, "lb_len or lb_gram is NULL");
    NMZ_TRY(pk_entities(n_entities));
    struct Prof {
        uint64_t len[32] = {};
        uint64_t gram[128] = {};
    } pa, pb;
    auto profile = [&](const uint64_t *t, const uint32_t *e, uint64_t len, const char *what, Prof &o) -> int {
        std::vector<uint64_t> last(n_entities, 0);
        std::vector<uint8_t> seen(n_entities, 0);
        for (uint64_t i = 0; i < len; ++i) {
            const uint32_t g = e[i];
            if (g == NMZ_NONE) continue;
            NMZ_CHECK(g < n_entities, std::string(what) + "'s element " + std::to_string(i) + " has entity id " +
                                          std::to_string(g) + ": ids are < n_entities (" + std::to_string(n_entities) +
                                          ") or NMZ_NONE");
            o.len[g % 32] += 1;
            const uint64_t prev = seen[g] ? last[g] : 0x9E3779B97F4A7C15ull;
            uint64_t x = prev + g;
            x ^= x >> 30, x *= 0xBF58476D1CE4E5B9ull, x ^= x >> 27, x *= 0x94D049BB133111EBull, x ^= x >> 31;
            x ^= t[i];
            x ^= x >> 30, x *= 0xBF58476D1CE4E5B9ull, x ^= x >> 27, x *= 0x94D049BB133111EBull, x ^= x >> 31;
            o.gram[x >> 57] += 1;
            seen[g] = 1;
            last[g] = t[i];
        }
        return NMZ_OK;
    };
    NMZ_TRY(profile(a, ea, n, "a", pa));
    NMZ_TRY(profile(b, eb, m, "b", pb));
    uint64_t l = 0, s = 0;
    for (int i = 0; i < 32; ++i) l += pa.len[i] > pb.len[i] ? pa.len[i] - pb.len[i] : pb.len[i] - pa.len[i];
    for (int h = 0; h < 128; ++h) {
        const uint64_t x = std::min<uint64_t>(pa.gram[h], 255), y = std::min<uint64_t>(pb.gram[h], 255);
        s += x > y ? x - y : y - x;
    }
    *lb_len = (uint32_t)std::min<uint64_t>(l, 0xFFFFFFFEull);
    *lb_gram = (uint32_t)((s + 3) / 4);
    return NMZ_OK;
}

int nmz_po_knn_plan_create(nmz_ctx *ctx, const uint64_t *off, const uint64_t *sym, const uint32_t *entity,
                           uint32_t n_traces, uint32_t n_entities, uint32_t band, uint64_t max_queries,
                           uint64_t max_query_elems, uint32_t opts, nmz_po_knn_plan **out) {
    return pk_plan_create_call(pk_band, PK_OPTS, ctx, off, sym, entity, n_traces, n_entities, band, max_queries,
                               max_query_elems, opts, out);
}

// The same plan for every band 0 .. 1,024: a band above 64 searches with K11w (ed_po_knn_wide.hip), a band <= 64 with
// K11b and so with the narrow entry point's bytes.
int nmz_po_knn_wide_plan_create(nmz_ctx *ctx, const uint64_t *off, const uint64_t *sym, const uint32_t *entity,
                                uint32_t n_traces, uint32_t n_entities, uint32_t band, uint64_t max_queries,
                                uint64_t max_query_elems, uint32_t opts, nmz_po_knn_plan **out) {
    return pk_plan_create_call(pkw_band, PKW_OPTS, ctx, off, sym, entity, n_traces, n_entities, band, max_queries,
                               max_query_elems, opts, out);
}

int nmz_po_knn_plan_destroy(nmz_po_knn_plan *plan) {
    if (!plan) return NMZ_OK;
    CtxGuard g(plan->ctx);
    NMZ_TRY(g.rc);
    pk_plan_destroy_locked(plan);
    return NMZ_OK;
}

int nmz_po_knn_plan_info(const nmz_po_knn_plan *plan, uint64_t *resident_bytes, uint32_t *blocks, uint32_t *waves) {
    NMZ_CHECK(plan != nullptr, "plan is NULL");
    if (resident_bytes) *resident_bytes = plan->resident_bytes;
    if (blocks) *blocks = plan->blocks;
    if (waves) *waves = plan->waves;
    return NMZ_OK;
}

int nmz_po_knn_query_dev(nmz_po_knn_plan *plan, const uint64_t *d_q_off, const uint64_t *d_q_sym,
                         const uint32_t *d_q_entity, const uint32_t *d_q_self, uint32_t n_queries, uint32_t k,
                         uint64_t *d_knn_keys, void *stream) {
    NMZ_CHECK(plan != nullptr, "plan is NULL");
    CtxGuard g(plan->ctx);
    NMZ_TRY(g.rc);
    return pk_enqueue(plan, stream ? (hipStream_t)stream : plan->ctx->stream, d_q_off, d_q_sym, d_q_entity, d_q_self,
                      n_queries, k, d_knn_keys);
}

int nmz_po_knn_query(nmz_po_knn_plan *plan, const uint64_t *q_off, const uint64_t *q_sym, const uint32_t *q_entity,
                     const uint32_t *q_self, uint32_t n_queries, uint32_t k, uint32_t *knn_id, uint32_t *knn_dist) {
    NMZ_CHECK(plan != nullptr, "plan is NULL");
    NMZ_TRY(pk_k(k));
    NMZ_TRY(pk_validate_queries(q_off, q_sym, q_entity, q_self, n_queries, plan->N, plan->G, knn_id, knn_dist));
    if (n_queries == 0) return NMZ_OK;  // nothing to write: no device either
    std::vector<uint64_t> boff;
    std::vector<uint32_t> bstart;
    NMZ_TRY(pk_batches(q_off, n_queries, plan->max_queries, plan->max_query_elems, boff, bstart));
    CtxGuard g(plan->ctx);
    NMZ_TRY(g.rc);
    HostCall call(plan->ctx);
    return pk_query_locked(plan, call, boff, bstart, q_off, q_sym, q_entity, q_self, n_queries, k, knn_id, knn_dist);
}

int nmz_po_knn(nmz_ctx *ctx, const uint64_t *off, const uint64_t *sym, const uint32_t *entity, uint32_t n_traces,
               uint32_t n_entities, const uint64_t *q_off, const uint64_t *q_sym, const uint32_t *q_entity,
               const uint32_t *q_self, uint32_t n_queries, uint32_t band, uint32_t k, uint32_t *knn_id,
               uint32_t *knn_dist) {
    return pk_one_shot(pk_band, ctx, off, sym, entity, n_traces, n_entities, q_off, q_sym, q_entity, q_self, n_queries,
                       band, k, knn_id, knn_dist);
}

int nmz_po_knn_wide(nmz_ctx *ctx, const uint64_t *off, const uint64_t *sym, const uint32_t *entity, uint32_t n_traces,
                    uint32_t n_entities, const uint64_t *q_off, const uint64_t *q_sym, const uint32_t *q_entity,
                    const uint32_t *q_self, uint32_t n_queries, uint32_t band, uint32_t k, uint32_t *knn_id,
                    uint32_t *knn_dist) {
    return pk_one_shot(pkw_band, ctx, off, sym, entity, n_traces, n_entities, q_off, q_sym, q_entity, q_self,
                       n_queries, band, k, knn_id, knn_dist);
}

int nmz_po_knn_counters(nmz_po_knn_plan *plan, uint64_t *out, void *stream) {
    return pk_counters(plan, out, PK_NCOUNTERS, stream);
}

// Words 4 .. 8: the entity steps K11w ran at C = 1, 2, 3, 5, 9 cells per thread; K11b leaves them at 0.
int nmz_po_knn_wide_counters(nmz_po_knn_plan *plan, uint64_t *out, void *stream) {
    return pk_counters(plan, out, PKW_NCOUNTERS, stream);
}

}  // extern "C"
