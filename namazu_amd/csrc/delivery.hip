// K1d -- delivery-order classes of replayable seeds (replayablepolicy.go:100-126 release times,
// cli/tools/visualize.go:51-136 trace equality).
//
// Replayable.QueueEvent releases every event at arrival + determineInterval(event), so a seed is a delivery order.
// For seed s (include/nmz_gpu.h has the full definition):
//     release[s][e] = arrival[e] + FNV1a64(seed_s || hint_e) % uint64(MaxInterval)      (0 when MaxInterval == 0)
//     pi_s          = the counted events sorted by (release asc, event index asc)
//     sig[s]        = the signature nmz_trace_signatures gives the trace delivered in that order (exact mode: ranks
//                     are positions in pi_s; PO mode: positions inside each entity's projection of pi_s)
//     min_gap_ns[s] = the smallest release difference of two neighbours of a compared sequence, gap_event its event
//
// Plan: the counted events are grouped by entity (a stable sort by entity id, so a segment keeps event-index order;
// exact mode is one segment). Per event in grouped order g the plan holds P^len, the arrival, the symbol, the
// original index and its segment's start; the hints are the affine table C[256][G] (FNV_hint(h0) = h0 * P^len +
// C_hint[h0 & 0xff]), row-major by low byte, so one seed's G corrections are one contiguous row.
//
// Kernel k_delivery_sweep<KIND, MODE>: one workgroup per seed at a time (grid-stride over the seeds), so the row
// index is uniform and the row, P^len and arrival reads are coalesced. Keys release << 12 | g (63 bits; g breaks
// ties by event index inside a segment) go to LDS with all-ones keys as padding, and a bitonic network sorts them:
//   DLV_EXACT    one segment: N = the power of two >= G slots, the whole network;
//   DLV_ALIGNED  PO mode, every segment in its own block of K slots (K = the power of two >= the longest segment),
//                when the blocks fit DLV_MAX_SLOTS: only the network's stages up to K run (independent sorts of short
//                segments, plain key compares), and rank = position inside the block;
//   DLV_GENERAL  PO mode otherwise (one long segment among many short ones): the whole network over N >= G slots
//                comparing (segment start of g, key); segments are contiguous in g, so after the sort segment j
//                occupies the positions it has in grouped order and rank = position - segment start.
// No per-entity counters in any mode. Each thread then mixes (sym, rank) for its positions and takes the gap to the
// previous position of the same segment; two block reductions (sums; lexicographic minimum of (gap, event)) give the
// 32-byte record, written in seed order. No per-seed arrays in registers: no scratch memory.
// m == 0 or no counted event: every seed has the same record, computed on the host at plan creation (k_delivery_fill).
#include <algorithm>
#include <string>
#include <vector>

#include "nmz_common.h"
#include "nmz_internal.h"
#include "order_dev.h"
#include "replayable_plan.h"
#include "sig_dev.h"

namespace nmz {

constexpr uint32_t DLV_MAX_EVENTS = NMZ_DELIVERY_MAX_EVENTS;
constexpr uint32_t DLV_IDX_BITS = 12;  // 4096 events
static_assert((1u << DLV_IDX_BITS) == DLV_MAX_EVENTS, "the key's index field");
constexpr uint32_t DLV_IDX_MASK = DLV_MAX_EVENTS - 1;
constexpr int64_t DLV_LIMIT = (int64_t)1 << 50;  // arrivals and MaxInterval: release < 2^51, key < 2^63
constexpr uint32_t DLV_MAX_ENTITY = 16384;       // nmz_unique_traces' bound on entity ids
constexpr uint64_t DLV_PAD = ~0ull;              // sorts last; its top bit marks it
constexpr uint32_t DLV_THREADS = 256;
constexpr uint32_t DLV_MAX_SLOTS = 4096;         // keys in LDS per seed (32 KB)
constexpr uint16_t DLV_NO_EVENT = 0xffffu;       // a padding slot of the aligned layout
enum : int { DLV_EXACT = 0, DLV_GENERAL = 1, DLV_ALIGNED = 2 };

struct DlvArgs {
    const uint64_t *h0;      // [S] seed prefix hashes
    const uint64_t *table;   // [256][G] hint corrections by FNV low byte
    const uint64_t *pn;      // [G] P^len
    const int64_t *arr;      // [G] arrival
    const uint64_t *sym;     // [G]
    const uint32_t *orig;    // [G] event index
    const uint16_t *ss;      // [G] first grouped position of the event's segment (DLV_GENERAL)
    const uint16_t *slot;    // [N] the grouped event of each slot, DLV_NO_EVENT for padding (DLV_ALIGNED)
    const ulonglong2 *keys;  // [RANK_KEYS] the signature's rank keys
    nmz_delivery_stats *stats;
    uint64_t S, m, mu;
    uint32_t G, N, K;        // counted events; slots (a multiple of K); the network's block (a power of two; K == N
                             // unless DLV_ALIGNED)
};

// a before b in (segment, release, index) order; pads last
template <bool PO>
__device__ __forceinline__ bool dlv_less(uint64_t a, uint64_t b, const uint16_t *ss) {
    if (PO) {
        const uint32_t sa = (a >> 63) ? 0xffffu : ss[a & DLV_IDX_MASK];
        const uint32_t sb = (b >> 63) ? 0xffffu : ss[b & DLV_IDX_MASK];
        if (sa != sb) return sa < sb;
    }
    return a < b;
}

template <int KIND, int MODE>
__global__ __launch_bounds__(DLV_THREADS) void k_delivery_sweep(const DlvArgs A) {
    constexpr bool PO = MODE == DLV_GENERAL;  // the compare looks the segments up
    extern __shared__ uint64_t dlv_lds[];
    __shared__ uint64_t red_a[DLV_THREADS / 64], red_b[DLV_THREADS / 64];
    __shared__ int64_t red_g[DLV_THREADS / 64];
    __shared__ uint32_t red_e[DLV_THREADS / 64];
    uint64_t *key = dlv_lds;                                        // [N]
    uint16_t *ss = reinterpret_cast<uint16_t *>(dlv_lds + A.N);     // [G] (DLV_GENERAL)
    const uint32_t tid = threadIdx.x, T = blockDim.x, G = A.G, N = A.N, K = A.K;
    if (PO)
        for (uint32_t i = tid; i < G; i += T) ss[i] = A.ss[i];
    for (uint64_t s = blockIdx.x; s < A.S; s += gridDim.x) {
        const uint64_t h = A.h0[s];
        const uint64_t *__restrict__ row = A.table + (size_t)(h & 0xffu) * G;
        for (uint32_t i = tid; i < N; i += T) {
            uint64_t k = DLV_PAD;
            const uint32_t g = MODE == DLV_ALIGNED ? A.slot[i] : (i < G ? i : DLV_NO_EVENT);
            if (g != DLV_NO_EVENT) {  // g < G
                const uint64_t d = order_mod<KIND>(h * A.pn[g] + row[g], A.m, A.mu);
                k = ((uint64_t)(A.arr[g] + (int64_t)d) << DLV_IDX_BITS) | g;
            }
            key[i] = k;
        }
        __syncthreads();
        for (uint32_t k = 2; k <= K; k <<= 1) {
            for (uint32_t j = k >> 1; j > 0; j >>= 1) {
                for (uint32_t t = tid; t < (N >> 1); t += T) {
                    const uint32_t lo = ((t & ~(j - 1)) << 1) | (t & (j - 1)), hi = lo + j;
                    const uint64_t a = key[lo], b = key[hi];
                    const bool asc = (lo & k & (K - 1)) == 0;  // the last stage sorts every block upwards
                    if (asc ? dlv_less<PO>(b, a, ss) : dlv_less<PO>(a, b, ss)) {
                        key[lo] = b;
                        key[hi] = a;
                    }
                }
                __syncthreads();
            }
        }
        uint64_t acc1 = 0, acc2 = 0;
        int64_t mg = INT64_MAX;
        uint32_t me = NMZ_NONE;
        for (uint32_t p = tid; p < (MODE == DLV_ALIGNED ? N : G); p += T) {
            const uint64_t k = key[p];
            if (MODE == DLV_ALIGNED && (k >> 63)) continue;  // padding at the end of a block
            const uint32_t g = (uint32_t)k & DLV_IDX_MASK;
            const uint32_t s0 = MODE == DLV_ALIGNED ? (p & ~(K - 1)) : PO ? ss[g] : 0u;
            uint64_t a, b;
            mix2k(A.sym[g], A.keys[p - s0], a, b);
            acc1 += a;
            acc2 += b;
            if (p > s0) {
                const int64_t gap = (int64_t)(k >> DLV_IDX_BITS) - (int64_t)(key[p - 1] >> DLV_IDX_BITS);
                const uint32_t ev = A.orig[g];
                if (gap < mg || (gap == mg && ev < me)) {
                    mg = gap;
                    me = ev;
                }
            }
        }
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) {
            acc1 += __shfl_xor(acc1, o, 64);
            acc2 += __shfl_xor(acc2, o, 64);
            const int64_t og = __shfl_xor(mg, o, 64);
            const uint32_t oe = __shfl_xor(me, o, 64);
            if (og < mg || (og == mg && oe < me)) {
                mg = og;
                me = oe;
            }
        }
        if ((tid & 63) == 0) {
            red_a[tid >> 6] = acc1;
            red_b[tid >> 6] = acc2;
            red_g[tid >> 6] = mg;
            red_e[tid >> 6] = me;
        }
        __syncthreads();  // also: every read of key[] is done before the next seed's keys are stored
        if (tid == 0) {
            for (uint32_t w = 1; w < (T >> 6); ++w) {
                acc1 += red_a[w];
                acc2 += red_b[w];
                if (red_g[w] < mg || (red_g[w] == mg && red_e[w] < me)) {
                    mg = red_g[w];
                    me = red_e[w];
                }
            }
            nmz_delivery_stats st;
            st.sig_lo = sig_final_lo(acc1, G);
            st.sig_hi = sig_final_hi(acc2, G);
            st.min_gap_ns = mg;
            st.gap_event = me;
            st.n_counted = G;
            A.stats[s] = st;
        }
    }
}

// every seed's record is the same (m == 0: the order is the plan's; or nothing is counted)
__global__ void k_delivery_fill(nmz_delivery_stats *__restrict__ stats, uint64_t S, const nmz_delivery_stats v) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < S) stats[i] = v;
}

// ---- classes over the stats ------------------------------------------------------------------------------------

__global__ void k_dlv_unpack(const nmz_delivery_stats *__restrict__ stats, uint32_t n, uint64_t *__restrict__ sig,
                             long long *__restrict__ best, uint32_t *__restrict__ rep) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    sig[2 * (uint64_t)i] = stats[i].sig_lo;
    sig[2 * (uint64_t)i + 1] = stats[i].sig_hi;
    best[i] = INT64_MIN;
    if (rep) rep[i] = NMZ_NONE;
}

// pass 1: the largest gap of each class on its head's slot; the heads are counted (one atomic per wave)
__global__ void k_dlv_best_gap(const nmz_delivery_stats *__restrict__ stats, const uint32_t *__restrict__ first,
                               uint32_t n, long long *__restrict__ best, uint32_t *__restrict__ n_classes) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    const bool in = i < n;
    const uint32_t h = in ? first[i] : 0u;
    if (in) atomicMax(&best[h], (long long)stats[i].min_gap_ns);
    if (n_classes) {
        const uint64_t heads = __builtin_amdgcn_ballot_w64(in && h == i);
        if ((threadIdx.x & 63) == 0 && heads) atomicAdd(n_classes, (uint32_t)__popcll(heads));
    }
}

// pass 2: among the members attaining it, the smallest index
__global__ void k_dlv_rep(const nmz_delivery_stats *__restrict__ stats, const uint32_t *__restrict__ first, uint32_t n,
                          const long long *__restrict__ best, uint32_t *__restrict__ rep) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t h = first[i];
    if ((long long)stats[i].min_gap_ns == best[h]) atomicMin(&rep[h], i);
}

static int delivery_classes_locked(nmz_ctx *ctx, const nmz_delivery_stats *d_stats, uint32_t n, uint32_t *d_first,
                                   uint32_t *d_rep, uint32_t *d_n_classes, hipStream_t st) {
    NMZ_CHECK(n <= 0x7fffffffu, "at most 2^31-1 signatures per call");
    if (d_n_classes) NMZ_HIP(hipMemsetAsync(d_n_classes, 0, 4, st));
    if (n == 0) return NMZ_OK;
    NMZ_CHECK(d_stats && d_first, "NULL argument");
    uint64_t *sig;
    long long *best;
    ScratchLayout lay;
    lay.add(&sig, 2 * (size_t)n).add(&best, n);
    NMZ_TRY(lay.bind(ctx->buf[SLOT_DELIVERY_CLASSES]));
    const unsigned g = ceil_div(n, 256);
    hipLaunchKernelGGL(k_dlv_unpack, dim3(g), dim3(256), 0, st, d_stats, n, sig, best, d_rep);
    NMZ_HIP(hipGetLastError());
    NMZ_TRY(classes_launch(ctx, sig, n, d_first, st));
    if (d_rep || d_n_classes) {
        hipLaunchKernelGGL(k_dlv_best_gap, dim3(g), dim3(256), 0, st, d_stats, d_first, n, best, d_n_classes);
        NMZ_HIP(hipGetLastError());
    }
    if (d_rep) {
        hipLaunchKernelGGL(k_dlv_rep, dim3(g), dim3(256), 0, st, d_stats, d_first, n, best, d_rep);
        NMZ_HIP(hipGetLastError());
    }
    return NMZ_OK;
}

// ---- host side -------------------------------------------------------------------------------------------------

// the limits of nmz_gpu.h, shared by the host decision and the plan
static int delivery_validate(const uint32_t *hint_off, const uint8_t *hint_bytes, uint32_t E, int64_t max_interval,
                             const int64_t *arrival, const uint64_t *sym, const uint32_t *entity) {
    NMZ_CHECK(E >= 1 && E <= DLV_MAX_EVENTS, "n_events must be in [1, 4096]");
    NMZ_CHECK(max_interval >= 0 && max_interval <= DLV_LIMIT, "max_interval_ns must be in [0, 2^50]");
    NMZ_CHECK(hint_off && arrival && sym, "hint_off, arrival_ns or sym is NULL");
    for (uint32_t e = 0; e < E; ++e) {
        NMZ_CHECK(arrival[e] >= 0 && arrival[e] <= DLV_LIMIT,
                  "arrival_ns[" + std::to_string(e) + "] must be in [0, 2^50]");
        NMZ_CHECK(hint_off[e] <= hint_off[e + 1], "hint offsets must not decrease");
        NMZ_CHECK(hint_off[e] == hint_off[e + 1] || hint_bytes, "hint_bytes is NULL");
        NMZ_CHECK(!entity || entity[e] == NMZ_NONE || entity[e] < DLV_MAX_ENTITY,
                  "entity[" + std::to_string(e) + "] must be < 16384 or NMZ_NONE");
    }
    return NMZ_OK;
}

// One seed by the definition (validated inputs): plain FNV byte loop from the prefix h0, %, std::sort, per-entity
// counters. order / release may be nullptr.
static void delivery_one(uint64_t h0, const uint32_t *hint_off, const uint8_t *hint_bytes, uint32_t E, uint64_t m,
                         const int64_t *arrival, const uint64_t *sym, const uint32_t *entity,
                         nmz_delivery_stats *stats, uint32_t *order, int64_t *release) {
    std::vector<int64_t> rel(E);
    std::vector<uint32_t> idx;
    idx.reserve(E);
    for (uint32_t e = 0; e < E; ++e) {
        int64_t d = 0;  // :101-104
        if (m != 0) {
            uint64_t h = h0;
            for (uint32_t b = hint_off[e]; b < hint_off[e + 1]; ++b) h = fnv_step(h, hint_bytes[b]);
            d = (int64_t)(h % m);
        }
        rel[e] = arrival[e] + d;
        if (!entity || entity[e] != NMZ_NONE) idx.push_back(e);
    }
    std::sort(idx.begin(), idx.end(),
              [&](uint32_t a, uint32_t b) { return rel[a] != rel[b] ? rel[a] < rel[b] : a < b; });
    std::vector<uint32_t> cnt(entity ? DLV_MAX_ENTITY : 1, 0u);
    std::vector<int64_t> last(entity ? DLV_MAX_ENTITY : 1, 0);
    uint64_t acc1 = 0, acc2 = 0;
    nmz_delivery_stats s{0, 0, INT64_MAX, NMZ_NONE, (uint32_t)idx.size()};
    for (uint32_t e : idx) {
        const uint32_t en = entity ? entity[e] : 0u;
        const uint32_t rank = cnt[en]++;
        uint64_t a, b;
        mix2k(sym[e], make_ulonglong2(rank_key_a(rank), rank_key_b(rank)), a, b);
        acc1 += a;
        acc2 += b;
        if (rank > 0) {
            const int64_t gap = rel[e] - last[en];
            if (gap < s.min_gap_ns || (gap == s.min_gap_ns && e < s.gap_event)) {
                s.min_gap_ns = gap;
                s.gap_event = e;
            }
        }
        last[en] = rel[e];
    }
    s.sig_lo = sig_final_lo(acc1, s.n_counted);
    s.sig_hi = sig_final_hi(acc2, s.n_counted);
    if (stats) *stats = s;
    if (order)
        for (uint32_t i = 0; i < E; ++i) order[i] = i < idx.size() ? idx[i] : NMZ_NONE;
    if (release)
        for (uint32_t e = 0; e < E; ++e) release[e] = rel[e];
}

}  // namespace nmz

struct nmz_replayable_delivery_plan {
    nmz_ctx *ctx = nullptr;
    uint32_t n_counted = 0;  // G
    uint32_t net = 0;        // slots N
    int mode = 0;            // DLV_EXACT, DLV_GENERAL or DLV_ALIGNED
    bool fixed = false;      // every seed has the record `same`
    nmz_delivery_stats same{};
    int kind = 0;
    uint64_t m = 0, mu = 0;
    uint64_t max_seeds = 0;
    nmz::DevBuf mem;  // the tables, the per-event arrays, the seeds' prefix hashes and their bucket counts
    nmz::DlvArgs args{};
    uint32_t *d_rows = nullptr;
    uint64_t *d_h0 = nullptr;
    // the streams the plan's sweeps were enqueued on, each with an event after its latest sweep (destroy waits)
    struct Use {
        hipStream_t st;
        hipEvent_t ev;
    };
    std::vector<Use> uses;
};

namespace nmz {

static void delivery_plan_destroy_locked(nmz_replayable_delivery_plan *p) {
    for (auto &u : p->uses) {
        (void)hipEventSynchronize(u.ev);
        (void)hipEventDestroy(u.ev);
    }
    p->mem.release();
    delete p;
}

static int delivery_plan_create_locked(nmz_ctx *ctx, const uint32_t *hint_off, const uint8_t *hint_bytes, uint32_t E,
                                       int64_t max_interval, const int64_t *arrival, const uint64_t *sym,
                                       const uint32_t *entity, uint64_t max_seeds,
                                       nmz_replayable_delivery_plan **out) {
    NMZ_TRY(delivery_validate(hint_off, hint_bytes, E, max_interval, arrival, sym, entity));
    NMZ_CHECK(max_seeds < (1ULL << 32), "at most 2^32-1 seeds per sweep");
    // counted events grouped by entity; stable, so a segment keeps event-index order (the tie rule)
    std::vector<uint32_t> grp;
    grp.reserve(E);
    for (uint32_t e = 0; e < E; ++e)
        if (!entity || entity[e] != NMZ_NONE) grp.push_back(e);
    if (entity)
        std::stable_sort(grp.begin(), grp.end(), [&](uint32_t a, uint32_t b) { return entity[a] < entity[b]; });
    const uint32_t G = (uint32_t)grp.size();
    auto *p = new nmz_replayable_delivery_plan();
    p->ctx = ctx;
    p->mem.pool = &ctx->pool;
    p->n_counted = G;
    p->m = (uint64_t)max_interval;  // uint64(r.MaxInterval), replayablepolicy.go:110
    p->kind = order_kind(p->m);
    p->mu = order_mu(p->m);
    p->max_seeds = max_seeds;
    p->fixed = p->m == 0 || G == 0;
    if (p->fixed)  // no seed enters: the delays are 0, or nothing is counted
        delivery_one(FNV_OFFSET, hint_off, hint_bytes, E, p->m, arrival, sym, entity, &p->same, nullptr, nullptr);
    p->net = 2;
    while (p->net < G) p->net <<= 1;
    uint32_t K = p->net;
    p->mode = entity ? DLV_GENERAL : DLV_EXACT;
    std::vector<uint16_t> slot;
    if (entity && G) {
        // segments (start, length) in grouped order; aligned blocks when they fit
        std::vector<std::pair<uint32_t, uint32_t>> segs;
        for (uint32_t g = 0; g < G; ++g) {
            if (g == 0 || entity[grp[g - 1]] != entity[grp[g]]) segs.push_back({g, 0u});
            ++segs.back().second;
        }
        uint32_t longest = 0;
        for (auto &sg : segs) longest = std::max(longest, sg.second);
        uint32_t kb = 2;
        while (kb < longest) kb <<= 1;
        if ((uint64_t)segs.size() * kb <= DLV_MAX_SLOTS) {
            p->mode = DLV_ALIGNED;
            K = kb;
            p->net = (uint32_t)segs.size() * kb;
            slot.assign(p->net, DLV_NO_EVENT);
            for (size_t b = 0; b < segs.size(); ++b)
                for (uint32_t r = 0; r < segs[b].second; ++r) slot[b * kb + r] = (uint16_t)(segs[b].first + r);
        }
    }
    if (slot.empty()) slot.assign(1, DLV_NO_EVENT);
    // host build: G hints x 256 low bytes (no table when no seed enters)
    const uint32_t Gp = G ? G : 1;
    std::vector<uint64_t> table(p->fixed ? 1 : (size_t)256 * G), pn(Gp), sy(Gp);
    std::vector<int64_t> ar(Gp);
    std::vector<uint32_t> orig(Gp);
    std::vector<uint16_t> ss(Gp);
    for (uint32_t g = 0; g < G; ++g) {
        const uint32_t e = grp[g];
        const uint32_t b0 = hint_off[e], b1 = hint_off[e + 1];
        pn[g] = fnv_pow(b1 - b0);
        ar[g] = arrival[e];
        sy[g] = sym[e];
        orig[g] = e;
        ss[g] = (uint16_t)((entity && g > 0 && entity[grp[g - 1]] == entity[e]) ? ss[g - 1] : (entity ? g : 0));
        if (!p->fixed)
            for (uint32_t L = 0; L < 256; ++L) {
                uint64_t h = L;
                for (uint32_t i = b0; i < b1; ++i) h = fnv_step(h, hint_bytes[i]);
                table[(size_t)L * G + g] = h - (uint64_t)L * pn[g];
            }
    }
    const size_t ns = max_seeds ? max_seeds : 1;
    uint64_t *d_table, *d_pn, *d_sym;
    int64_t *d_arr;
    uint32_t *d_orig;
    uint16_t *d_ss, *d_slot;
    ScratchLayout lay;
    lay.add(&d_table, table.size()).add(&d_pn, Gp).add(&d_arr, Gp).add(&d_sym, Gp).add(&d_orig, Gp).add(&d_ss, Gp);
    lay.add(&d_slot, slot.size()).add(&p->d_h0, ns).add(&p->d_rows, bucket_hist_u32(ns));
    int rc = lay.bind(p->mem);
    const ulonglong2 *keys = nullptr;
    if (rc == NMZ_OK) rc = sig_rank_keys(ctx, &keys);
    if (rc != NMZ_OK) {
        p->mem.release();
        delete p;
        return rc;
    }
    p->args = DlvArgs{p->d_h0, d_table, d_pn, d_arr, d_sym, d_orig, d_ss, d_slot, keys,
                      nullptr, 0,      p->m, p->mu, G,      p->net, K};
    hipStream_t st = ctx->stream;
    hipError_t e = hipMemcpyAsync(d_table, table.data(), table.size() * 8, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(d_pn, pn.data(), (size_t)Gp * 8, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(d_arr, ar.data(), (size_t)Gp * 8, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(d_sym, sy.data(), (size_t)Gp * 8, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(d_orig, orig.data(), (size_t)Gp * 4, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(d_ss, ss.data(), (size_t)Gp * 2, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(d_slot, slot.data(), slot.size() * 2, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);  // the host arrays go out of scope; sweeps may take any stream
    if (e != hipSuccess) {
        (void)hipStreamSynchronize(st);
        p->mem.release();
        delete p;
        return fail(NMZ_EHIP, std::string("delivery plan upload: ") + hipGetErrorString(e));
    }
    *out = p;
    return NMZ_OK;
}

// enqueue one sweep: seeds = the device CSR, or (d_soff == nullptr) the decimal strings of dec_lo .. dec_lo + S - 1
static int delivery_run(nmz_replayable_delivery_plan *p, hipStream_t st, const uint32_t *d_soff,
                        const uint8_t *d_sbytes, uint64_t dec_lo, uint64_t S, nmz_delivery_stats *d_stats) {
    NMZ_CHECK(S <= p->max_seeds, "more seeds than the plan was created for");
    if (S == 0) return NMZ_OK;
    NMZ_CHECK(d_stats != nullptr, "d_stats is NULL");
    nmz_replayable_delivery_plan::Use *u = nullptr;
    for (auto &x : p->uses)
        if (x.st == st) u = &x;
    if (!u) {
        hipEvent_t ev;
        NMZ_HIP(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        p->uses.push_back({st, ev});
        u = &p->uses.back();
    }
    int rc = NMZ_OK;
    if (p->fixed) {
        hipLaunchKernelGGL(k_delivery_fill, dim3(ceil_div(S, 256)), dim3(256), 0, st, d_stats, S, p->same);
        if (hipGetLastError() != hipSuccess) rc = fail(NMZ_EHIP, "k_delivery_fill launch failed");
    } else {
        rc = seed_prefix_launch(st, d_soff, d_sbytes, dec_lo, S, p->d_h0, p->d_rows);
        if (rc == NMZ_OK) {
            KernelTimer kt(p->ctx, st, "delivery_sweep");
            DlvArgs a = p->args;
            a.stats = d_stats;
            a.S = S;
            // half the network's size in threads, whole waves; workgroups for every wave slot of the device
            const uint32_t T = std::min(DLV_THREADS, (std::max(64u, p->net / 2) + 63u) & ~63u);
            const size_t lds = (size_t)p->net * 8 +
                               (p->mode == DLV_GENERAL ? (((size_t)p->n_counted * 2 + 7) & ~size_t(7)) : 0);
            const uint64_t slots = (uint64_t)std::max(p->ctx->n_cu, 1) * (2048 / T);
            const unsigned blocks = (unsigned)std::min<uint64_t>(S, slots);
#define NMZ_K1D(KIND, MODE) \
    hipLaunchKernelGGL((k_delivery_sweep<KIND, MODE>), dim3(blocks), dim3(T), lds, st, a)
#define NMZ_K1D_KIND(MODE)                                 \
    switch (p->kind) {                                    \
        case ORD_SMALL: NMZ_K1D(ORD_SMALL, MODE); break;   \
        case ORD_MID: NMZ_K1D(ORD_MID, MODE); break;       \
        default: NMZ_K1D(ORD_WIDE, MODE); break;           \
    }
            if (p->mode == DLV_ALIGNED) {
                NMZ_K1D_KIND(DLV_ALIGNED)
            } else if (p->mode == DLV_GENERAL) {
                NMZ_K1D_KIND(DLV_GENERAL)
            } else {
                NMZ_K1D_KIND(DLV_EXACT)
            }
#undef NMZ_K1D_KIND
#undef NMZ_K1D
            if (hipGetLastError() != hipSuccess) rc = fail(NMZ_EHIP, "k_delivery_sweep launch failed");
        }
    }
    NMZ_HIP(hipEventRecord(u->ev, st));
    return rc;
}

// the host-pointer sweeps: plan + upload + sweep + classes + results, synchronous
static int delivery_sweep_host(nmz_ctx *ctx, const uint32_t *seed_off, const uint8_t *seed_bytes, uint64_t seed_lo,
                               uint64_t n_seeds, const uint32_t *hint_off, const uint8_t *hint_bytes,
                               uint32_t n_events, int64_t max_interval_ns, const int64_t *arrival_ns,
                               const uint64_t *sym, const uint32_t *entity, nmz_delivery_stats *stats,
                               uint32_t *first_equal, uint32_t *class_rep, uint32_t *n_classes, bool decimal) {
    NMZ_CHECK(ctx != nullptr, "ctx is NULL");
    NMZ_CHECK(decimal || n_seeds == 0 || seed_off, "seed_off is NULL");
    const bool classes = first_equal || class_rep || n_classes;
    NMZ_CHECK(n_seeds < (1ULL << 32), "at most 2^32-1 seeds per call");
    NMZ_CHECK(!classes || n_seeds < (1ULL << 31), "at most 2^31-1 seeds per call with classes");
    CtxGuard g(ctx);
    NMZ_TRY(g.rc);
    HostCall call(ctx);
    nmz_replayable_delivery_plan *plan = nullptr;
    NMZ_TRY(delivery_plan_create_locked(ctx, hint_off, hint_bytes, n_events, max_interval_ns, arrival_ns, sym, entity,
                                        n_seeds, &plan));
    call.own_plan<delivery_plan_destroy_locked>(plan);
    hipStream_t st = ctx->stream;
    uint64_t sbytes;
    NMZ_TRY(seed_csr_bytes(seed_off, seed_bytes, n_seeds, decimal, &sbytes));
    uint32_t *d_soff, *d_first, *d_rep, *d_nc;
    uint8_t *d_sb;
    nmz_delivery_stats *d_stats;
    ScratchLayout lay;
    lay.add(&d_soff, n_seeds + 1).add(&d_sb, sbytes + 1).add(&d_stats, n_seeds + 1);
    lay.add(&d_first, n_seeds + 1).add(&d_rep, n_seeds + 1).add(&d_nc, 1);
    NMZ_TRY(lay.bind(ctx->buf[SLOT_TARGET_DELIVERY_HOST]));
    NMZ_TRY(upload_seeds(d_soff, d_sb, seed_off, seed_bytes, n_seeds, decimal, st));
    NMZ_TRY(delivery_run(plan, st, decimal ? nullptr : d_soff, d_sb, seed_lo, n_seeds, d_stats));
    if (classes) {
        KernelTimer kt(ctx, st, "delivery_classes");
        NMZ_TRY(delivery_classes_locked(ctx, d_stats, (uint32_t)n_seeds, d_first, class_rep ? d_rep : nullptr,
                                        n_classes ? d_nc : nullptr, st));
    }
    if (stats) NMZ_TRY(copy_d2h(stats, d_stats, n_seeds, st));
    if (first_equal) NMZ_TRY(copy_d2h(first_equal, d_first, n_seeds, st));
    if (class_rep) NMZ_TRY(copy_d2h(class_rep, d_rep, n_seeds, st));
    if (n_classes) NMZ_TRY(copy_d2h(n_classes, d_nc, 1, st));
    return call.done();
}

}  // namespace nmz

using namespace nmz;

extern "C" {

int nmz_replayable_delivery_host(const uint8_t *seed, uint32_t seed_len, const uint32_t *hint_off,
                                 const uint8_t *hint_bytes, uint32_t n_events, int64_t max_interval_ns,
                                 const int64_t *arrival_ns, const uint64_t *sym, const uint32_t *entity,
                                 nmz_delivery_stats *stats, uint32_t *order, int64_t *release_ns) {
    NMZ_CHECK(seed_len == 0 || seed, "seed is NULL");
    NMZ_TRY(delivery_validate(hint_off, hint_bytes, n_events, max_interval_ns, arrival_ns, sym, entity));
    uint64_t h0 = FNV_OFFSET;
    for (uint32_t i = 0; i < seed_len; ++i) h0 = fnv_step(h0, seed[i]);
    delivery_one(h0, hint_off, hint_bytes, n_events, (uint64_t)max_interval_ns, arrival_ns, sym, entity, stats, order,
                 release_ns);
    return NMZ_OK;
}

int nmz_replayable_delivery_plan_create(nmz_ctx *ctx, const uint32_t *hint_off, const uint8_t *hint_bytes,
                                        uint32_t n_events, int64_t max_interval_ns, const int64_t *arrival_ns,
                                        const uint64_t *sym, const uint32_t *entity, uint64_t max_seeds,
                                        nmz_replayable_delivery_plan **out) {
    NMZ_CHECK(ctx && out, "NULL argument");
    *out = nullptr;
    CtxGuard g(ctx);
    NMZ_TRY(g.rc);
    return delivery_plan_create_locked(ctx, hint_off, hint_bytes, n_events, max_interval_ns, arrival_ns, sym, entity,
                                       max_seeds, out);
}

int nmz_replayable_delivery_plan_destroy(nmz_replayable_delivery_plan *plan) {
    if (!plan) return NMZ_OK;
    CtxGuard g(plan->ctx);
    NMZ_TRY(g.rc);
    delivery_plan_destroy_locked(plan);
    return NMZ_OK;
}

int nmz_replayable_delivery_sweep_decimal_dev(nmz_replayable_delivery_plan *plan, uint64_t seed_lo, uint64_t n_seeds,
                                              nmz_delivery_stats *d_stats, void *stream) {
    NMZ_CHECK(plan != nullptr, "plan is NULL");
    CtxGuard g(plan->ctx);
    NMZ_TRY(g.rc);
    return delivery_run(plan, stream ? (hipStream_t)stream : plan->ctx->stream, nullptr, nullptr, seed_lo, n_seeds,
                        d_stats);
}

int nmz_replayable_delivery_sweep_dev(nmz_replayable_delivery_plan *plan, const uint32_t *d_seed_off,
                                      const uint8_t *d_seed_bytes, uint64_t n_seeds, nmz_delivery_stats *d_stats,
                                      void *stream) {
    NMZ_CHECK(plan != nullptr, "plan is NULL");
    NMZ_CHECK(n_seeds == 0 || d_seed_off, "d_seed_off is NULL");
    CtxGuard g(plan->ctx);
    NMZ_TRY(g.rc);
    return delivery_run(plan, stream ? (hipStream_t)stream : plan->ctx->stream, d_seed_off, d_seed_bytes, 0, n_seeds,
                        d_stats);
}

int nmz_delivery_classes_dev(nmz_ctx *ctx, const nmz_delivery_stats *d_stats, uint32_t n, uint32_t *d_first_equal,
                             uint32_t *d_class_rep, uint32_t *d_n_classes, void *stream) {
    NMZ_CHECK(ctx != nullptr, "ctx is NULL");
    CtxGuard g(ctx);
    NMZ_TRY(g.rc);
    return delivery_classes_locked(ctx, d_stats, n, d_first_equal, d_class_rep, d_n_classes,
                                   stream ? (hipStream_t)stream : ctx->stream);
}

int nmz_sig_classes_dev(nmz_ctx *ctx, const uint64_t *d_sig, uint32_t n, uint32_t *d_first_equal, void *stream) {
    NMZ_CHECK(ctx != nullptr, "ctx is NULL");
    NMZ_CHECK(n <= 0x7fffffffu, "at most 2^31-1 signatures per call");
    CtxGuard g(ctx);
    NMZ_TRY(g.rc);
    if (n == 0) return NMZ_OK;
    NMZ_CHECK(d_sig && d_first_equal, "NULL argument");
    return classes_launch(ctx, d_sig, n, d_first_equal, stream ? (hipStream_t)stream : ctx->stream);
}

int nmz_replayable_delivery_sweep(nmz_ctx *ctx, const uint32_t *seed_off, const uint8_t *seed_bytes, uint64_t n_seeds,
                                  const uint32_t *hint_off, const uint8_t *hint_bytes, uint32_t n_events,
                                  int64_t max_interval_ns, const int64_t *arrival_ns, const uint64_t *sym,
                                  const uint32_t *entity, nmz_delivery_stats *stats, uint32_t *first_equal,
                                  uint32_t *class_rep, uint32_t *n_classes) {
    return delivery_sweep_host(ctx, seed_off, seed_bytes, 0, n_seeds, hint_off, hint_bytes, n_events, max_interval_ns,
                               arrival_ns, sym, entity, stats, first_equal, class_rep, n_classes, false);
}

int nmz_replayable_delivery_sweep_decimal(nmz_ctx *ctx, uint64_t seed_lo, uint64_t n_seeds, const uint32_t *hint_off,
                                          const uint8_t *hint_bytes, uint32_t n_events, int64_t max_interval_ns,
                                          const int64_t *arrival_ns, const uint64_t *sym, const uint32_t *entity,
                                          nmz_delivery_stats *stats, uint32_t *first_equal, uint32_t *class_rep,
                                          uint32_t *n_classes) {
    return delivery_sweep_host(ctx, nullptr, nullptr, seed_lo, n_seeds, hint_off, hint_bytes, n_events,
                               max_interval_ns, arrival_ns, sym, entity, stats, first_equal, class_rep, n_classes,
                               true);
}

}  // extern "C"
