// K1t -- nearest-order sweep: replayable seeds ranked by the closeness of their delivery order to a recorded run
// (replayablepolicy.go:100-126 release times; historystorage/naive/naive.go:235-257 prefix search).
//
// Releases, the delivery order pi_s and the compared sequences are the delivery sweep's (delivery.hip) over the
// counted events (target_pos != NMZ_NONE and, in PO mode, entity != NMZ_NONE). Per seed (include/nmz_gpu.h):
//     n_discordant = pairs of one compared sequence delivered the other way round than target_pos orders them
//     prefix_len   = leading events of the target order that are all in place (rank in pi_s == rank by target_pos)
//     n_in_place, min_gap_ns, gap_event
//
// Plan: the delivery sweep's (events grouped by entity, tables C[256][G], P^len, arrivals; the layouts DLV_EXACT,
// DLV_ALIGNED and DLV_GENERAL) plus pd[g] = the slot of grouped event g when its segment is laid out in target
// order | its dense target position << 16.
//
// Kernel k_target_sweep<KIND, MODE>: one workgroup per seed at a time, grid-striding. Keys release << 12 | g are
// computed in grouped order (coalesced row, P^len and arrival reads) and stored to LDS slot pd[g], i.e. in target
// order inside each segment. A merge sort by ranking then sorts by key: at level l every key binary-searches the
// sibling run of 2^l slots, its output slot is its offset in its own run plus the number of smaller siblings, and a
// key of a right run adds 2^l - count (the left keys it overtakes) to the seed's inversion sum. The exchanges that
// take the target order to the key order are the discordant pairs. Real keys are distinct; padding (all ones, after
// each segment's events) never moves, so it is written once to both buffers and skipped. Aligned blocks stop at
// level K; the general layout compares (segment start, key), so keys of different segments never exchange.
// After the last level position == pd[g]'s slot means "in place"; a minimum over the out-of-place events' dense
// target positions is prefix_len; neighbour differences give the gap as in K1d.
// LDS: two key buffers (16 N bytes, 64 KB at N = 4096) + the segment starts in the general layout; pd[] is read
// from global memory (16 KB at most, one gather per event), so two workgroups fit a CU. No scratch memory.
// The top-k turns the stats into nmz_sched_stats keys (k_target_topk_keys) and runs topk_select (procset.hip's
// pattern).
#include <algorithm>
#include <string>
#include <vector>

#include "nmz_common.h"
#include "nmz_internal.h"
#include "order_dev.h"
#include "replayable_plan.h"

namespace nmz {

constexpr uint32_t TGT_MAX_EVENTS = NMZ_DELIVERY_MAX_EVENTS;
constexpr uint32_t TGT_IDX_BITS = 12;
static_assert((1u << TGT_IDX_BITS) == TGT_MAX_EVENTS, "the key's index field");
constexpr uint32_t TGT_IDX_MASK = TGT_MAX_EVENTS - 1;
constexpr int64_t TGT_LIMIT = (int64_t)1 << 50;  // arrivals and MaxInterval: release < 2^51, key < 2^63
constexpr uint32_t TGT_MAX_ENTITY = 16384;
constexpr uint64_t TGT_PAD = ~0ull;              // sorts last; its top bit marks it
constexpr uint32_t TGT_THREADS = 1024;           // at most; 4 slots per thread
constexpr uint32_t TGT_WAVES = TGT_THREADS / 64;
constexpr uint32_t TGT_MAX_SLOTS = 4096;         // keys per buffer (32 KB)
constexpr uint16_t TGT_NO_EVENT = 0xffffu;
constexpr size_t TGT_LDS_CU = 160 * 1024;
enum : int { TGT_EXACT = 0, TGT_GENERAL = 1, TGT_ALIGNED = 2 };  // the delivery sweep's layouts

struct TgtArgs {
    const uint64_t *h0;      // [S] seed prefix hashes
    const uint64_t *table;   // [256][G] hint corrections by FNV low byte
    const uint64_t *pn;      // [G] P^len
    const int64_t *arr;      // [G] arrival
    const uint32_t *orig;    // [G] event index
    const uint16_t *ss;      // [G] first slot of the event's segment (TGT_GENERAL)
    const uint16_t *slot;    // [N] the grouped event of each slot in target order, TGT_NO_EVENT for padding
    const uint32_t *pd;      // [G] slot in target order | dense target position << 16
    nmz_target_stats *stats;
    uint64_t S, m, mu;
    uint32_t G, N, K;        // counted events; slots (a multiple of K); the merge's block (a power of two; K == N
                             // unless TGT_ALIGNED)
};

// y before x in (segment, release, index) order; x is a real key of segment sx, y may be padding
template <bool PO>
__device__ __forceinline__ bool tgt_less(uint64_t y, uint64_t x, uint32_t sx, const uint16_t *ss) {
    if (PO) {
        const uint32_t sy = (y >> 63) ? 0xffffu : ss[y & TGT_IDX_MASK];
        if (sy != sx) return sy < sx;
    }
    return y < x;
}

template <int KIND, int MODE>
__global__ __launch_bounds__(TGT_THREADS) void k_target_sweep(const TgtArgs A) {
    constexpr bool PO = MODE == TGT_GENERAL;  // the compare looks the segments up
    extern __shared__ uint64_t tgt_lds[];
    __shared__ uint32_t red_d[TGT_WAVES], red_n[TGT_WAVES], red_p[TGT_WAVES], red_e[TGT_WAVES];
    __shared__ int64_t red_g[TGT_WAVES];
    const uint32_t tid = threadIdx.x, T = blockDim.x, G = A.G, N = A.N, K = A.K;
    uint64_t *const buf0 = tgt_lds, *const buf1 = tgt_lds + N;               // [N] each
    uint16_t *ss = reinterpret_cast<uint16_t *>(tgt_lds + 2 * (size_t)N);  // [G] (TGT_GENERAL)
    const uint32_t n_live = MODE == TGT_ALIGNED ? N : G;  // slots that may hold an event
    if (PO)
        for (uint32_t i = tid; i < G; i += T) ss[i] = A.ss[i];
    // padding keeps its slot through every level: once, in both buffers
    for (uint32_t i = tid; i < N; i += T)
        if (A.slot[i] == TGT_NO_EVENT) {
            buf0[i] = TGT_PAD;
            buf1[i] = TGT_PAD;
        }
    for (uint64_t s = blockIdx.x; s < A.S; s += gridDim.x) {
        const uint64_t h = A.h0[s];
        const uint64_t *__restrict__ row = A.table + (size_t)(h & 0xffu) * G;
        for (uint32_t g = tid; g < G; g += T) {
            const uint64_t d = order_mod<KIND>(h * A.pn[g] + row[g], A.m, A.mu);
            buf0[A.pd[g] & 0xffffu] = ((uint64_t)(A.arr[g] + (int64_t)d) << TGT_IDX_BITS) | g;
        }
        __syncthreads();
        uint64_t *src = buf0, *dst = buf1;
        uint32_t disc = 0;
        for (uint32_t R = 1; R < K; R <<= 1) {
            for (uint32_t i = tid; i < n_live; i += T) {
                const uint64_t x = src[i];
                if (x >> 63) continue;
                const uint32_t sx = PO ? ss[x & TGT_IDX_MASK] : 0u;
                const uint32_t sb = (i & ~(R - 1)) ^ R;  // the sibling run
                uint32_t c = 0;
                for (uint32_t hs = R >> 1; hs > 0; hs >>= 1) c += tgt_less<PO>(src[sb + c + hs - 1], x, sx, ss) ? hs : 0u;
                c += tgt_less<PO>(src[sb + c], x, sx, ss) ? 1u : 0u;
                dst[(i & ~(2 * R - 1)) + (i & (R - 1)) + c] = x;
                if (i & R) disc += R - c;
            }
            __syncthreads();
            uint64_t *t = src;
            src = dst;
            dst = t;
        }
        uint32_t nin = 0, pmin = G, me = NMZ_NONE;
        int64_t mg = INT64_MAX;
        for (uint32_t p = tid; p < n_live; p += T) {
            const uint64_t k = src[p];
            if (k >> 63) continue;  // padding at the end of a block
            const uint32_t g = (uint32_t)k & TGT_IDX_MASK;
            const uint32_t pd = A.pd[g];
            if ((pd & 0xffffu) == p)
                ++nin;
            else
                pmin = min(pmin, pd >> 16);
            const uint32_t s0 = MODE == TGT_ALIGNED ? (p & ~(K - 1)) : PO ? ss[g] : 0u;
            if (p > s0) {
                const int64_t gap = (int64_t)(k >> TGT_IDX_BITS) - (int64_t)(src[p - 1] >> TGT_IDX_BITS);
                if (gap <= mg) {
                    const uint32_t ev = A.orig[g];
                    if (gap < mg || ev < me) {
                        mg = gap;
                        me = ev;
                    }
                }
            }
        }
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) {
            disc += __shfl_xor(disc, o, 64);
            nin += __shfl_xor(nin, o, 64);
            pmin = min(pmin, (uint32_t)__shfl_xor(pmin, o, 64));
            const int64_t og = __shfl_xor(mg, o, 64);
            const uint32_t oe = __shfl_xor(me, o, 64);
            if (og < mg || (og == mg && oe < me)) {
                mg = og;
                me = oe;
            }
        }
        if ((tid & 63) == 0) {
            red_d[tid >> 6] = disc;
            red_n[tid >> 6] = nin;
            red_p[tid >> 6] = pmin;
            red_g[tid >> 6] = mg;
            red_e[tid >> 6] = me;
        }
        __syncthreads();  // also: every read of the keys is done before the next seed's keys are stored
        if (tid == 0) {
            for (uint32_t w = 1; w < (T >> 6); ++w) {
                disc += red_d[w];
                nin += red_n[w];
                pmin = min(pmin, red_p[w]);
                if (red_g[w] < mg || (red_g[w] == mg && red_e[w] < me)) {
                    mg = red_g[w];
                    me = red_e[w];
                }
            }
            nmz_target_stats st;
            st.n_discordant = disc;
            st.prefix_len = pmin;
            st.min_gap_ns = mg;
            st.gap_event = me;
            st.n_in_place = nin;
            A.stats[s] = st;
        }  // the next seed's barriers come before its reduction slots are written
    }
}

// every seed's record is the same (m == 0: the order is the plan's; or nothing is counted)
__global__ void k_target_fill(nmz_target_stats *__restrict__ stats, uint64_t S, const nmz_target_stats v) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < S) stats[i] = v;
}

// the stats as keys of the schedule top-k (topk.hip: n_fault desc, sum_delay desc as int64, seed asc). The
// selection's coarse key keeps the top 48 bits of the sign-flipped sum: min_gap_ns in [0, 2^51] and INT64_MAX keep
// their order under it (a monotone map); n_fault >= 0xffff saturates it, and the selection then ranks exactly.
__global__ __launch_bounds__(256) void k_target_topk_keys(const nmz_target_stats *__restrict__ stats, uint64_t n,
                                                          uint32_t n_pairs, int rank_mode,
                                                          nmz_sched_stats *__restrict__ keys) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const nmz_target_stats t = stats[i];
    const uint32_t conc = n_pairs - t.n_discordant;
    nmz_sched_stats k;
    stats_empty(k);
    if (rank_mode == NMZ_TARGET_RANK_PREFIX) {
        k.n_fault = t.prefix_len;
        k.sum_delay_ns = conc;
        k.first_fault = t.n_in_place;
    } else {
        k.n_fault = conc;
        k.sum_delay_ns = (uint64_t)t.min_gap_ns;
        k.first_fault = t.prefix_len;
    }
    keys[i] = k;
}

// ---- host side -------------------------------------------------------------------------------------------------

static bool tgt_counted(const uint32_t *entity, const uint32_t *target_pos, uint32_t e) {
    return target_pos[e] != NMZ_NONE && (!entity || entity[e] != NMZ_NONE);
}

// the limits of nmz_gpu.h (the delivery sweep's, and distinct target positions), shared by the host decision and
// the plan
static int target_validate(const uint32_t *hint_off, const uint8_t *hint_bytes, uint32_t E, int64_t max_interval,
                           const int64_t *arrival, const uint32_t *entity, const uint32_t *target_pos) {
    NMZ_CHECK(E >= 1 && E <= TGT_MAX_EVENTS, "n_events must be in [1, 4096]");
    NMZ_CHECK(max_interval >= 0 && max_interval <= TGT_LIMIT, "max_interval_ns must be in [0, 2^50]");
    NMZ_CHECK(hint_off && arrival && target_pos, "hint_off, arrival_ns or target_pos is NULL");
    std::vector<uint32_t> tp;
    for (uint32_t e = 0; e < E; ++e) {
        NMZ_CHECK(arrival[e] >= 0 && arrival[e] <= TGT_LIMIT,
                  "arrival_ns[" + std::to_string(e) + "] must be in [0, 2^50]");
        NMZ_CHECK(hint_off[e] <= hint_off[e + 1], "hint offsets must not decrease");
        NMZ_CHECK(hint_off[e] == hint_off[e + 1] || hint_bytes, "hint_bytes is NULL");
        NMZ_CHECK(!entity || entity[e] == NMZ_NONE || entity[e] < TGT_MAX_ENTITY,
                  "entity[" + std::to_string(e) + "] must be < 16384 or NMZ_NONE");
        if (tgt_counted(entity, target_pos, e)) tp.push_back(target_pos[e]);
    }
    std::sort(tp.begin(), tp.end());
    for (size_t i = 1; i < tp.size(); ++i)
        NMZ_CHECK(tp[i - 1] != tp[i],
                  "target_pos " + std::to_string(tp[i]) + " appears twice among the counted events");
    return NMZ_OK;
}

// inversions of v (pairs i < j with v[i] > v[j]) by a merge count; v ends sorted
static uint64_t tgt_inversions(std::vector<uint32_t> &v) {
    std::vector<uint32_t> tmp(v.size());
    uint64_t inv = 0;
    for (size_t w = 1; w < v.size(); w *= 2) {
        for (size_t lo = 0; lo < v.size(); lo += 2 * w) {
            const size_t mid = std::min(lo + w, v.size()), hi = std::min(lo + 2 * w, v.size());
            size_t a = lo, b = mid, o = lo;
            while (a < mid && b < hi) {
                if (v[b] < v[a]) {
                    inv += mid - a;
                    tmp[o++] = v[b++];
                } else {
                    tmp[o++] = v[a++];
                }
            }
            while (a < mid) tmp[o++] = v[a++];
            while (b < hi) tmp[o++] = v[b++];
        }
        v.swap(tmp);
        tmp.resize(v.size());
    }
    return inv;
}

// One seed by the definition (validated inputs): plain FNV byte loop from the prefix h0, %, std::sort, the
// sequences walked one by one. n_counted / n_pairs may be nullptr.
static void target_one(uint64_t h0, const uint32_t *hint_off, const uint8_t *hint_bytes, uint32_t E, uint64_t m,
                       const int64_t *arrival, const uint32_t *entity, const uint32_t *target_pos,
                       nmz_target_stats *stats, uint32_t *n_counted, uint32_t *n_pairs) {
    std::vector<int64_t> rel(E);
    std::vector<uint32_t> idx, all_tp;
    for (uint32_t e = 0; e < E; ++e) {
        int64_t d = 0;  // :101-104
        if (m != 0) {
            uint64_t h = h0;
            for (uint32_t b = hint_off[e]; b < hint_off[e + 1]; ++b) h = fnv_step(h, hint_bytes[b]);
            d = (int64_t)(h % m);
        }
        rel[e] = arrival[e] + d;
        if (tgt_counted(entity, target_pos, e)) {
            idx.push_back(e);
            all_tp.push_back(target_pos[e]);
        }
    }
    std::sort(idx.begin(), idx.end(),
              [&](uint32_t a, uint32_t b) { return rel[a] != rel[b] ? rel[a] < rel[b] : a < b; });
    std::sort(all_tp.begin(), all_tp.end());
    // the compared sequences: the whole order, or each entity's projection of it
    std::vector<std::vector<uint32_t>> seqs;
    if (!entity) {
        seqs.push_back(idx);
    } else {
        std::vector<int32_t> where(TGT_MAX_ENTITY, -1);
        for (uint32_t e : idx) {
            if (where[entity[e]] < 0) {
                where[entity[e]] = (int32_t)seqs.size();
                seqs.emplace_back();
            }
            seqs[where[entity[e]]].push_back(e);
        }
    }
    nmz_target_stats s{0, (uint32_t)idx.size(), INT64_MAX, NMZ_NONE, 0};
    uint64_t pairs = 0;
    for (const auto &q : seqs) {
        const size_t n = q.size();
        pairs += (uint64_t)n * (n - 1) / 2;
        std::vector<uint32_t> tp(n);
        for (size_t i = 0; i < n; ++i) tp[i] = target_pos[q[i]];
        std::vector<uint32_t> sorted = tp;
        s.n_discordant += (uint32_t)tgt_inversions(sorted);  // leaves the sequence's target positions sorted
        for (size_t i = 0; i < n; ++i) {
            const size_t trank = std::lower_bound(sorted.begin(), sorted.end(), tp[i]) - sorted.begin();
            if (trank == i) {
                ++s.n_in_place;
            } else {
                const uint32_t dense = (uint32_t)(std::lower_bound(all_tp.begin(), all_tp.end(), tp[i]) - all_tp.begin());
                s.prefix_len = std::min(s.prefix_len, dense);
            }
            if (i > 0) {
                const int64_t gap = rel[q[i]] - rel[q[i - 1]];
                if (gap < s.min_gap_ns || (gap == s.min_gap_ns && q[i] < s.gap_event)) {
                    s.min_gap_ns = gap;
                    s.gap_event = q[i];
                }
            }
        }
    }
    if (stats) *stats = s;
    if (n_counted) *n_counted = (uint32_t)idx.size();
    if (n_pairs) *n_pairs = (uint32_t)pairs;
}

}  // namespace nmz

struct nmz_replayable_target_plan {
    nmz_ctx *ctx = nullptr;
    uint32_t n_counted = 0;  // G
    uint32_t n_pairs = 0;
    uint32_t net = 0;        // slots N
    int mode = 0;            // TGT_EXACT, TGT_GENERAL or TGT_ALIGNED
    bool fixed = false;      // every seed has the record `same`
    nmz_target_stats same{};
    int kind = 0;
    uint64_t m = 0, mu = 0;
    uint64_t max_seeds = 0;
    nmz::DevBuf mem;      // the tables, the per-event arrays, the seeds' prefix hashes and their bucket counts
    nmz::DevBuf scratch;  // top-k: the stats (when the caller takes none), the keys, the selection's lists
    nmz::TgtArgs args{};
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

static void target_plan_destroy_locked(nmz_replayable_target_plan *p) {
    for (auto &u : p->uses) {
        (void)hipEventSynchronize(u.ev);
        (void)hipEventDestroy(u.ev);
    }
    p->mem.release();
    p->scratch.release();
    delete p;
}

static int target_plan_create_locked(nmz_ctx *ctx, const uint32_t *hint_off, const uint8_t *hint_bytes, uint32_t E,
                                     int64_t max_interval, const int64_t *arrival, const uint32_t *entity,
                                     const uint32_t *target_pos, uint64_t max_seeds,
                                     nmz_replayable_target_plan **out) {
    NMZ_TRY(target_validate(hint_off, hint_bytes, E, max_interval, arrival, entity, target_pos));
    NMZ_CHECK(max_seeds < (1ULL << 32), "at most 2^32-1 seeds per sweep");
    // counted events grouped by entity; stable, so a segment keeps event-index order (the tie rule)
    std::vector<uint32_t> grp;
    grp.reserve(E);
    for (uint32_t e = 0; e < E; ++e)
        if (tgt_counted(entity, target_pos, e)) grp.push_back(e);
    if (entity)
        std::stable_sort(grp.begin(), grp.end(), [&](uint32_t a, uint32_t b) { return entity[a] < entity[b]; });
    const uint32_t G = (uint32_t)grp.size();
    auto *p = new nmz_replayable_target_plan();
    p->ctx = ctx;
    p->mem.pool = &ctx->pool;
    p->scratch.pool = &ctx->pool;
    p->n_counted = G;
    p->m = (uint64_t)max_interval;  // uint64(r.MaxInterval), replayablepolicy.go:110
    p->kind = order_kind(p->m);
    p->mu = order_mu(p->m);
    p->max_seeds = max_seeds;
    p->fixed = p->m == 0 || G == 0;
    // the constants, and (no seed enters: the delays are 0, or nothing is counted) every seed's record
    target_one(FNV_OFFSET, hint_off, hint_bytes, E, p->fixed ? p->m : 0, arrival, entity, target_pos, &p->same, nullptr,
               &p->n_pairs);
    p->net = 2;
    while (p->net < G) p->net <<= 1;
    uint32_t K = p->net, kb = 0;
    p->mode = entity ? TGT_GENERAL : TGT_EXACT;
    // segments (start, length) in grouped order; aligned blocks when they fit
    std::vector<std::pair<uint32_t, uint32_t>> segs;
    for (uint32_t g = 0; g < G; ++g) {
        if (g == 0 || (entity && entity[grp[g - 1]] != entity[grp[g]])) segs.push_back({g, 0u});
        ++segs.back().second;
    }
    if (entity && G) {
        uint32_t longest = 0;
        for (auto &sg : segs) longest = std::max(longest, sg.second);
        kb = 2;
        while (kb < longest) kb <<= 1;
        if ((uint64_t)segs.size() * kb <= TGT_MAX_SLOTS) {
            p->mode = TGT_ALIGNED;
            K = kb;
            p->net = (uint32_t)segs.size() * kb;
        }
    }
    // slots in target order inside each segment, and every event's dense target position
    const uint32_t Gp = G ? G : 1;
    std::vector<uint16_t> slot(p->net, TGT_NO_EVENT), ss(Gp);
    std::vector<uint32_t> pd(Gp), by_tp(grp);
    std::sort(by_tp.begin(), by_tp.end(), [&](uint32_t a, uint32_t b) { return target_pos[a] < target_pos[b]; });
    std::vector<uint32_t> dense(E, 0u);
    for (uint32_t i = 0; i < G; ++i) dense[by_tp[i]] = i;
    for (size_t b = 0; b < segs.size(); ++b) {
        const uint32_t g0 = segs[b].first, n = segs[b].second;
        const uint32_t s0 = p->mode == TGT_ALIGNED ? (uint32_t)b * kb : g0;
        std::vector<uint32_t> gs(n);
        for (uint32_t r = 0; r < n; ++r) gs[r] = g0 + r;
        std::sort(gs.begin(), gs.end(),
                  [&](uint32_t a, uint32_t c) { return target_pos[grp[a]] < target_pos[grp[c]]; });
        for (uint32_t r = 0; r < n; ++r) {
            slot[s0 + r] = (uint16_t)gs[r];
            pd[gs[r]] = (s0 + r) | (dense[grp[gs[r]]] << 16);
            ss[gs[r]] = (uint16_t)s0;
        }
    }
    // host build: G hints x 256 low bytes (no table when no seed enters)
    std::vector<uint64_t> table(p->fixed ? 1 : (size_t)256 * G), pn(Gp);
    std::vector<int64_t> ar(Gp);
    std::vector<uint32_t> orig(Gp);
    for (uint32_t g = 0; g < G; ++g) {
        const uint32_t e = grp[g];
        const uint32_t b0 = hint_off[e], b1 = hint_off[e + 1];
        pn[g] = fnv_pow(b1 - b0);
        ar[g] = arrival[e];
        orig[g] = e;
        if (!p->fixed)
            for (uint32_t L = 0; L < 256; ++L) {
                uint64_t h = L;
                for (uint32_t i = b0; i < b1; ++i) h = fnv_step(h, hint_bytes[i]);
                table[(size_t)L * G + g] = h - (uint64_t)L * pn[g];
            }
    }
    const size_t ns = max_seeds ? max_seeds : 1;
    uint64_t *d_table, *d_pn;
    int64_t *d_arr;
    uint32_t *d_orig, *d_pd;
    uint16_t *d_ss, *d_slot;
    ScratchLayout lay;
    lay.add(&d_table, table.size()).add(&d_pn, Gp).add(&d_arr, Gp).add(&d_orig, Gp).add(&d_pd, Gp).add(&d_ss, Gp);
    lay.add(&d_slot, slot.size()).add(&p->d_h0, ns).add(&p->d_rows, bucket_hist_u32(ns));
    int rc = lay.bind(p->mem);
    if (rc != NMZ_OK) {
        p->mem.release();
        delete p;
        return rc;
    }
    p->args = TgtArgs{p->d_h0, d_table, d_pn, d_arr, d_orig, d_ss, d_slot, d_pd, nullptr, 0, p->m, p->mu, G, p->net, K};
    hipStream_t st = ctx->stream;
    hipError_t e = hipMemcpyAsync(d_table, table.data(), table.size() * 8, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(d_pn, pn.data(), (size_t)Gp * 8, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(d_arr, ar.data(), (size_t)Gp * 8, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(d_orig, orig.data(), (size_t)Gp * 4, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(d_pd, pd.data(), (size_t)Gp * 4, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(d_ss, ss.data(), (size_t)Gp * 2, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(d_slot, slot.data(), slot.size() * 2, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);  // the host arrays go out of scope; sweeps may take any stream
    if (e != hipSuccess) {
        (void)hipStreamSynchronize(st);
        p->mem.release();
        delete p;
        return fail(NMZ_EHIP, std::string("target plan upload: ") + hipGetErrorString(e));
    }
    *out = p;
    return NMZ_OK;
}

template <int KIND, int MODE>
static int target_launch(const TgtArgs &a, unsigned blocks, uint32_t T, size_t lds, hipStream_t st) {
    if (lds > 32 * 1024)  // beyond the default dynamic LDS of a launch; per device, cheap to repeat
        NMZ_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(k_target_sweep<KIND, MODE>),
                                    hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL((k_target_sweep<KIND, MODE>), dim3(blocks), dim3(T), lds, st, a);
    return NMZ_OK;
}

template <int MODE>
static int target_launch_kind(int kind, const TgtArgs &a, unsigned blocks, uint32_t T, size_t lds, hipStream_t st) {
    switch (kind) {
        case ORD_SMALL: return target_launch<ORD_SMALL, MODE>(a, blocks, T, lds, st);
        case ORD_MID: return target_launch<ORD_MID, MODE>(a, blocks, T, lds, st);
        default: return target_launch<ORD_WIDE, MODE>(a, blocks, T, lds, st);
    }
}

// enqueue one sweep: seeds = the device CSR, or (d_soff == nullptr) the decimal strings of dec_lo .. dec_lo + S - 1
static int target_run(nmz_replayable_target_plan *p, hipStream_t st, const uint32_t *d_soff, const uint8_t *d_sbytes,
                      uint64_t dec_lo, uint64_t S, uint64_t seed0, int rank_mode, uint32_t k,
                      nmz_target_stats *d_stats, nmz_topk_entry *d_topk) {
    NMZ_CHECK(S <= p->max_seeds, "more seeds than the plan was created for");
    NMZ_CHECK(rank_mode == NMZ_TARGET_RANK_PAIRS || rank_mode == NMZ_TARGET_RANK_PREFIX,
              "rank_mode must be NMZ_TARGET_RANK_PAIRS or NMZ_TARGET_RANK_PREFIX");
    NMZ_CHECK(k <= 256, "top-k supports k <= 256");
    NMZ_CHECK(k == 0 || d_topk, "d_topk is NULL");
    if (S == 0 && k == 0) return NMZ_OK;
    NMZ_CHECK(d_stats || k, "d_stats is NULL and k is 0: nothing to compute");
    // the top-k's scratch, sized once for the plan (max_seeds, k = 256), so a later sweep never moves it
    nmz_sched_stats *d_keys = nullptr;
    nmz_topk_entry *d_lists = nullptr;
    if (k) {
        const size_t ns = p->max_seeds ? p->max_seeds : 1;
        nmz_target_stats *own;
        ScratchLayout lay;
        lay.add(&own, ns).add(&d_keys, ns).add(&d_lists, topk_scratch_entries(ns, 256));
        NMZ_TRY(lay.bind(p->scratch));
        if (!d_stats) d_stats = own;
    }
    nmz_replayable_target_plan::Use *u = nullptr;
    for (auto &x : p->uses)
        if (x.st == st) u = &x;
    if (!u) {
        hipEvent_t ev;
        NMZ_HIP(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        p->uses.push_back({st, ev});
        u = &p->uses.back();
    }
    int rc = NMZ_OK;
    if (S == 0) {
        // no seeds: the list is all sentinels
    } else if (p->fixed) {
        hipLaunchKernelGGL(k_target_fill, dim3(ceil_div(S, 256)), dim3(256), 0, st, d_stats, S, p->same);
        if (hipGetLastError() != hipSuccess) rc = fail(NMZ_EHIP, "k_target_fill launch failed");
    } else {
        rc = seed_prefix_launch(st, d_soff, d_sbytes, dec_lo, S, p->d_h0, p->d_rows);
        if (rc == NMZ_OK) {
            KernelTimer kt(p->ctx, st, "target_sweep");
            TgtArgs a = p->args;
            a.stats = d_stats;
            a.S = S;
            // a quarter of the slots in threads, whole waves; workgroups for every LDS and wave slot of the device
            const uint32_t T = std::min(TGT_THREADS, (std::max(64u, p->net / 4) + 63u) & ~63u);
            const size_t lds = (size_t)p->net * 16 +
                               (p->mode == TGT_GENERAL ? (((size_t)p->n_counted * 2 + 7) & ~size_t(7)) : 0);
            const uint64_t per_cu = std::max<uint64_t>(1, std::min<uint64_t>(2048 / T, TGT_LDS_CU / (lds + 512)));
            const unsigned blocks = (unsigned)std::min<uint64_t>(S, (uint64_t)std::max(p->ctx->n_cu, 1) * per_cu);
            if (p->mode == TGT_ALIGNED)
                rc = target_launch_kind<TGT_ALIGNED>(p->kind, a, blocks, T, lds, st);
            else if (p->mode == TGT_GENERAL)
                rc = target_launch_kind<TGT_GENERAL>(p->kind, a, blocks, T, lds, st);
            else
                rc = target_launch_kind<TGT_EXACT>(p->kind, a, blocks, T, lds, st);
            if (rc == NMZ_OK && hipGetLastError() != hipSuccess) rc = fail(NMZ_EHIP, "k_target_sweep launch failed");
        }
    }
    if (rc == NMZ_OK && k) {
        KernelTimer kt(p->ctx, st, "target_topk");
        if (S) {
            hipLaunchKernelGGL(k_target_topk_keys, dim3(ceil_div(S, 256)), dim3(256), 0, st, d_stats, S, p->n_pairs,
                               rank_mode, d_keys);
            if (hipGetLastError() != hipSuccess) rc = fail(NMZ_EHIP, "k_target_topk_keys launch failed");
        }
        if (rc == NMZ_OK) rc = topk_select(st, d_keys, S, seed0, k, d_lists, d_topk);
    }
    NMZ_HIP(hipEventRecord(u->ev, st));
    return rc;
}

// the host-pointer sweeps: plan + upload + sweep + top-k + results, synchronous
static int target_sweep_host(nmz_ctx *ctx, const uint32_t *seed_off, const uint8_t *seed_bytes, uint64_t seed_lo,
                             uint64_t n_seeds, const uint32_t *hint_off, const uint8_t *hint_bytes, uint32_t n_events,
                             int64_t max_interval_ns, const int64_t *arrival_ns, const uint32_t *entity,
                             const uint32_t *target_pos, int rank_mode, uint32_t k, nmz_target_stats *stats,
                             nmz_topk_entry *topk, uint32_t *n_counted, uint32_t *n_pairs, bool decimal) {
    NMZ_CHECK(ctx != nullptr, "ctx is NULL");
    NMZ_CHECK(decimal || n_seeds == 0 || seed_off, "seed_off is NULL");
    NMZ_CHECK(n_seeds < (1ULL << 32), "at most 2^32-1 seeds per call");
    NMZ_CHECK(k <= 256, "top-k supports k <= 256");
    if (!topk) k = 0;
    CtxGuard g(ctx);
    NMZ_TRY(g.rc);
    HostCall call(ctx);
    nmz_replayable_target_plan *plan = nullptr;
    NMZ_TRY(target_plan_create_locked(ctx, hint_off, hint_bytes, n_events, max_interval_ns, arrival_ns, entity,
                                      target_pos, n_seeds, &plan));
    call.own_plan<target_plan_destroy_locked>(plan);
    if (n_counted) *n_counted = plan->n_counted;
    if (n_pairs) *n_pairs = plan->n_pairs;
    hipStream_t st = ctx->stream;
    uint64_t sbytes;
    NMZ_TRY(seed_csr_bytes(seed_off, seed_bytes, n_seeds, decimal, &sbytes));
    uint32_t *d_soff;
    uint8_t *d_sb;
    nmz_target_stats *d_stats;
    nmz_topk_entry *d_tk;
    ScratchLayout lay;
    lay.add(&d_soff, n_seeds + 1).add(&d_sb, sbytes + 1).add(&d_stats, n_seeds + 1).add(&d_tk, k + 1);
    NMZ_TRY(lay.bind(ctx->buf[SLOT_TARGET_DELIVERY_HOST]));
    NMZ_TRY(upload_seeds(d_soff, d_sb, seed_off, seed_bytes, n_seeds, decimal, st));
    // the rank mode is checked even when there is nothing to rank
    NMZ_TRY(target_run(plan, st, decimal ? nullptr : d_soff, d_sb, seed_lo, n_seeds, decimal ? seed_lo : 0, rank_mode,
                       k, (stats || !k) ? d_stats : nullptr, d_tk));
    if (stats) NMZ_TRY(copy_d2h(stats, d_stats, n_seeds, st));
    NMZ_TRY(copy_d2h(topk, d_tk, k, st));
    return call.done();
}

}  // namespace nmz

using namespace nmz;

extern "C" {

int nmz_replayable_target_host(const uint8_t *seed, uint32_t seed_len, const uint32_t *hint_off,
                               const uint8_t *hint_bytes, uint32_t n_events, int64_t max_interval_ns,
                               const int64_t *arrival_ns, const uint32_t *entity, const uint32_t *target_pos,
                               nmz_target_stats *stats, uint32_t *n_counted, uint32_t *n_pairs) {
    NMZ_CHECK(seed_len == 0 || seed, "seed is NULL");
    NMZ_TRY(target_validate(hint_off, hint_bytes, n_events, max_interval_ns, arrival_ns, entity, target_pos));
    uint64_t h0 = FNV_OFFSET;
    for (uint32_t i = 0; i < seed_len; ++i) h0 = fnv_step(h0, seed[i]);
    target_one(h0, hint_off, hint_bytes, n_events, (uint64_t)max_interval_ns, arrival_ns, entity, target_pos, stats,
               n_counted, n_pairs);
    return NMZ_OK;
}

int nmz_replayable_target_plan_create(nmz_ctx *ctx, const uint32_t *hint_off, const uint8_t *hint_bytes,
                                      uint32_t n_events, int64_t max_interval_ns, const int64_t *arrival_ns,
                                      const uint32_t *entity, const uint32_t *target_pos, uint64_t max_seeds,
                                      nmz_replayable_target_plan **out) {
    NMZ_CHECK(ctx && out, "NULL argument");
    *out = nullptr;
    CtxGuard g(ctx);
    NMZ_TRY(g.rc);
    return target_plan_create_locked(ctx, hint_off, hint_bytes, n_events, max_interval_ns, arrival_ns, entity,
                                     target_pos, max_seeds, out);
}

int nmz_replayable_target_plan_destroy(nmz_replayable_target_plan *plan) {
    if (!plan) return NMZ_OK;
    CtxGuard g(plan->ctx);
    NMZ_TRY(g.rc);
    target_plan_destroy_locked(plan);
    return NMZ_OK;
}

int nmz_replayable_target_plan_info(const nmz_replayable_target_plan *plan, uint32_t *n_counted, uint32_t *n_pairs) {
    NMZ_CHECK(plan != nullptr, "plan is NULL");
    if (n_counted) *n_counted = plan->n_counted;
    if (n_pairs) *n_pairs = plan->n_pairs;
    return NMZ_OK;
}

int nmz_replayable_target_sweep_decimal_dev(nmz_replayable_target_plan *plan, uint64_t seed_lo, uint64_t n_seeds,
                                            int rank_mode, uint32_t k, nmz_target_stats *d_stats,
                                            nmz_topk_entry *d_topk, void *stream) {
    NMZ_CHECK(plan != nullptr, "plan is NULL");
    CtxGuard g(plan->ctx);
    NMZ_TRY(g.rc);
    return target_run(plan, stream ? (hipStream_t)stream : plan->ctx->stream, nullptr, nullptr, seed_lo, n_seeds,
                      seed_lo, rank_mode, k, d_stats, d_topk);
}

int nmz_replayable_target_sweep_dev(nmz_replayable_target_plan *plan, const uint32_t *d_seed_off,
                                    const uint8_t *d_seed_bytes, uint64_t n_seeds, uint64_t seed0, int rank_mode,
                                    uint32_t k, nmz_target_stats *d_stats, nmz_topk_entry *d_topk, void *stream) {
    NMZ_CHECK(plan != nullptr, "plan is NULL");
    NMZ_CHECK(n_seeds == 0 || d_seed_off, "d_seed_off is NULL");
    CtxGuard g(plan->ctx);
    NMZ_TRY(g.rc);
    return target_run(plan, stream ? (hipStream_t)stream : plan->ctx->stream, d_seed_off, d_seed_bytes, 0, n_seeds,
                      seed0, rank_mode, k, d_stats, d_topk);
}

int nmz_replayable_target_sweep(nmz_ctx *ctx, const uint32_t *seed_off, const uint8_t *seed_bytes, uint64_t n_seeds,
                                const uint32_t *hint_off, const uint8_t *hint_bytes, uint32_t n_events,
                                int64_t max_interval_ns, const int64_t *arrival_ns, const uint32_t *entity,
                                const uint32_t *target_pos, int rank_mode, uint32_t k, nmz_target_stats *stats,
                                nmz_topk_entry *topk, uint32_t *n_counted, uint32_t *n_pairs) {
    return target_sweep_host(ctx, seed_off, seed_bytes, 0, n_seeds, hint_off, hint_bytes, n_events, max_interval_ns,
                             arrival_ns, entity, target_pos, rank_mode, k, stats, topk, n_counted, n_pairs, false);
}

int nmz_replayable_target_sweep_decimal(nmz_ctx *ctx, uint64_t seed_lo, uint64_t n_seeds, const uint32_t *hint_off,
                                        const uint8_t *hint_bytes, uint32_t n_events, int64_t max_interval_ns,
                                        const int64_t *arrival_ns, const uint32_t *entity, const uint32_t *target_pos,
                                        int rank_mode, uint32_t k, nmz_target_stats *stats, nmz_topk_entry *topk,
                                        uint32_t *n_counted, uint32_t *n_pairs) {
    return target_sweep_host(ctx, nullptr, nullptr, seed_lo, n_seeds, hint_off, hint_bytes, n_events, max_interval_ns,
                             arrival_ns, entity, target_pos, rank_mode, k, stats, topk, n_counted, n_pairs, true);
}

}  // extern "C"
