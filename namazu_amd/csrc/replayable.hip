// K1 -- replayable-policy seed sweep (replayablepolicy.go:100-126).
//
//   delay(seed, event) = FNV1a64(seed || hint_e) % uint64(MaxInterval)
//
// Algorithm (MI355X-native, not the reference's per-event hasher):
//  1. Per event, FNV over the hint bytes is an affine map of the incoming
//     state h0 with a correction that depends only on h0's low byte:
//         FNV_hint(h0) = h0 * P^len + C_e[h0 & 0xff]         (mod 2^64)
//     A plan kernel builds C_e[L] for all 256 L (one table row per L).
//  2. Seeds are FNV-hashed once (prefix state h0) and bucketed by h0 & 0xff,
//     so every lane of a wave reads the same table row: table reads are
//     wave-uniform scalar loads.
//  3. Events are grouped by hint length; per (seed, length class) the lane
//     precomputes H = h0*P^len, Hm = H mod m and Hm' = (Hm + 2^64 mod m) mod m:
//         h = H + C (mod 2^64),  carry = C > ~H
//         h mod m = (carry ? Hm' : Hm) + (C mod m)   (one conditional -m)
//  4. Within every (row L, class) segment the table is sorted by C, so the
//     carry is monotone in the position: carry <=> pos >= k(seed), with k
//     found by one binary search per (seed, segment). Per decision the carry
//     is a single compare of a running position counter -- no 64-bit add.
//  5. Per-seed statistics (sum, max with first-index argmax) accumulate in
//     registers; the argmax tie-break uses the key (t << 32 | ~e) so the
//     sorted event order still yields the first original index.
//
// This unit: the plan (table kernels, plan_create), the dispatch over the kernel families (replayable_stats), the
// trace pipeline and the C ABI. The families: seed prefixes (step 2) in replayable_seeds.hip; the per-decision
// sweeps (steps 3-5 as written) in replayable_pd.hip; the statistics kernels, which answer a whole segment per
// seed from the same algebra, in replayable_oq.hip and replayable_wt.hip. replayable_plan.h is what they share.
#include <algorithm>
#include <cstring>
#include <cstdlib>
#include <numeric>
#include <string>
#include <vector>

#include "nmz_common.h"
#include "nmz_internal.h"
#include "replayable_plan.h"

namespace nmz {

// ---------------------------------------------------------------------------
// plan: per-(L, event) correction table
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_replayable_table(const uint32_t *__restrict__ hoff,
                                                          const uint8_t *__restrict__ hbytes,
                                                          const uint32_t *__restrict__ perm, uint32_t E,
                                                          uint64_t m, int fast, uint4 *__restrict__ table) {
    const uint32_t pos = blockIdx.x;  // sorted position
    const uint32_t L = threadIdx.x;
    const uint32_t e = perm[pos];
    const uint32_t b0 = hoff[e], b1 = hoff[e + 1];
    uint64_t h = L;
    for (uint32_t i = b0; i < b1; ++i) h = fnv_step(h, hbytes[i]);
    const uint64_t C = h - (uint64_t)L * fnv_pow(b1 - b0);
    const uint32_t cm = fast ? (uint32_t)(C % m) : 0u;
    table[(uint64_t)L * E + pos] = make_uint4((uint32_t)C, (uint32_t)(C >> 32), cm, ~e);
}

// Sort every (row L, class) segment of the table by C (ascending, ties by
// position): rank by counting over the segment through LDS tiles, then
// scatter. O(n_class^2) per row -- ~1e10 compares at E = 4096, well under a ms.
__global__ __launch_bounds__(256) void k_replayable_table_sort(const uint4 *__restrict__ tmp,
                                                               const ClassInfo *__restrict__ classes,
                                                               uint32_t n_classes, uint32_t E,
                                                               uint4 *__restrict__ table) {
    __shared__ uint2 tile[256];
    const uint32_t L = blockIdx.y;
    const uint32_t p0 = blockIdx.x * 256;
    const uint32_t p = p0 + threadIdx.x;
    const uint4 *__restrict__ row = tmp + (uint64_t)L * E;
    uint32_t cs = 0, ce = 0, lo = UINT32_MAX, hi = 0;
    for (uint32_t c = 0; c < n_classes; ++c) {
        const uint32_t a = classes[c].start, b = a + classes[c].count;
        if (p >= a && p < b) cs = a, ce = b;
        // union of the classes this block touches
        if (b > p0 && a < min(E, p0 + 256)) lo = min(lo, a), hi = max(hi, b);
    }
    const uint4 x = p < E ? row[p] : make_uint4(0, 0, 0, 0);
    const uint64_t cx = ((uint64_t)x.y << 32) | x.x;
    uint32_t rank = 0;
    for (uint32_t j0 = lo; j0 < hi; j0 += 256) {
        __syncthreads();
        if (j0 + threadIdx.x < hi) {
            const uint4 y = row[j0 + threadIdx.x];
            tile[threadIdx.x] = make_uint2(y.x, y.y);
        }
        __syncthreads();
        const uint32_t jn = min(256u, hi - j0);
        for (uint32_t jj = 0; jj < jn; ++jj) {
            const uint32_t j = j0 + jj;
            const uint64_t cj = ((uint64_t)tile[jj].y << 32) | tile[jj].x;
            rank += (j >= cs && j < ce && (cj < cx || (cj == cx && j < p))) ? 1u : 0u;
        }
    }
    if (p < E) table[(uint64_t)L * E + cs + rank] = x;
}

// Sort one (class, row L) segment per workgroup in LDS by (C, position) -- the stable C order of
// k_replayable_table_sort -- then gather the table entries in that order. C is an FNV-derived 64-bit value, so a
// counting sort on its top 12 bits leaves ~n/4096 entries per bucket; each bucket is finished by one thread
// (insertion sort). A segment whose largest bucket exceeds SEG_BUCKET_MAX (adversarial C values) takes a bitonic
// sort instead. Segments of up to SEG_SORT_MAX entries; larger classes keep the counting kernel above.
constexpr uint32_t SEG_SORT_MAX = 4096;
constexpr uint32_t SEG_BUCKETS = 4096;
constexpr uint32_t SEG_BUCKET_MAX = 32;

__global__ __launch_bounds__(1024) void k_replayable_table_segsort(const uint4 *__restrict__ tmp,
                                                                   const ClassInfo *__restrict__ classes, uint32_t E,
                                                                   uint4 *__restrict__ table) {
    __shared__ uint64_t key[SEG_SORT_MAX];
    __shared__ uint16_t pos[SEG_SORT_MAX];
    __shared__ uint32_t cnt[SEG_BUCKETS];
    __shared__ uint32_t wsum[16], maxb;
    const ClassInfo ci = classes[blockIdx.x];
    const uint32_t L = blockIdx.y, n = ci.count, t = threadIdx.x;
    if (n > SEG_SORT_MAX || n == 0) return;
    const uint4 *__restrict__ src = tmp + (uint64_t)L * E + ci.start;
    for (uint32_t i = t; i < SEG_BUCKETS; i += blockDim.x) cnt[i] = 0;
    if (t == 0) maxb = 0;
    __syncthreads();
    uint64_t mine[SEG_SORT_MAX / 1024];
#pragma unroll
    for (uint32_t r = 0; r < SEG_SORT_MAX / 1024; ++r) {
        const uint32_t i = r * 1024 + t;
        mine[r] = 0;
        if (i < n) {
            const uint4 q = src[i];
            mine[r] = ((uint64_t)q.y << 32) | q.x;
            atomicAdd(&cnt[mine[r] >> 52], 1u);
        }
    }
    __syncthreads();
    // exclusive scan of the 4096 counts: 4 per thread, wave scans, then the 16 wave totals
    uint32_t c4[4], tot = 0, mx = 0;
#pragma unroll
    for (uint32_t r = 0; r < 4; ++r) {
        c4[r] = cnt[4 * t + r];
        tot += c4[r];
        mx = max(mx, c4[r]);
    }
    const uint32_t lane = t & 63, w = t >> 6;
    uint32_t inc = tot;
    for (uint32_t o = 1; o < 64; o <<= 1) {
        const uint32_t v = __shfl_up(inc, o, 64);
        if (lane >= o) inc += v;
    }
    if (lane == 63) wsum[w] = inc;
    atomicMax(&maxb, mx);
    __syncthreads();
    uint32_t base = inc - tot;
    for (uint32_t j = 0; j < w; ++j) base += wsum[j];
#pragma unroll
    for (uint32_t r = 0; r < 4; ++r) {
        cnt[4 * t + r] = base;  // bucket start, advanced by the scatter below
        base += c4[r];
    }
    __syncthreads();
    if (maxb <= SEG_BUCKET_MAX) {
#pragma unroll
        for (uint32_t r = 0; r < SEG_SORT_MAX / 1024; ++r) {
            const uint32_t i = r * 1024 + t;
            if (i < n) {
                const uint32_t slot = atomicAdd(&cnt[mine[r] >> 52], 1u);
                key[slot] = mine[r];
                pos[slot] = (uint16_t)i;
            }
        }
        __syncthreads();
        // cnt[b] is now the end of bucket b; one thread per bucket sorts its few entries by (C, position)
        for (uint32_t b = t; b < SEG_BUCKETS; b += blockDim.x) {
            const uint32_t e1 = cnt[b], e0 = b ? cnt[b - 1] : 0;
            for (uint32_t i = e0 + 1; i < e1; ++i) {
                const uint64_t k = key[i];
                const uint16_t p = pos[i];
                uint32_t j = i;
                while (j > e0 && (key[j - 1] > k || (key[j - 1] == k && pos[j - 1] > p))) {
                    key[j] = key[j - 1];
                    pos[j] = pos[j - 1];
                    --j;
                }
                key[j] = k;
                pos[j] = p;
            }
        }
        __syncthreads();
    } else {  // bitonic sort of (C, position) padded to a power of two
        uint32_t p2 = 1;
        while (p2 < n) p2 <<= 1;
        for (uint32_t i = t; i < p2; i += blockDim.x) {
            key[i] = i < n ? (((uint64_t)src[i].y << 32) | src[i].x) : UINT64_MAX;
            pos[i] = (uint16_t)i;
        }
        __syncthreads();
        for (uint32_t k = 2; k <= p2; k <<= 1) {
            for (uint32_t j = k >> 1; j > 0; j >>= 1) {
                const uint32_t lj = 31 - __builtin_clz(j);
                for (uint32_t p = t; p < p2 / 2; p += blockDim.x) {
                    const uint32_t i = ((p >> lj) << (lj + 1)) | (p & (j - 1)), l = i + j;
                    const uint64_t ki = key[i], kl = key[l];
                    const uint32_t pi = pos[i], pl = pos[l];
                    const bool gt = ki > kl || (ki == kl && pi > pl);
                    if (((i & k) == 0) == gt) {  // ascending half: swap if i > l; descending half: if i < l
                        key[i] = kl;
                        key[l] = ki;
                        pos[i] = (uint16_t)pl;
                        pos[l] = (uint16_t)pi;
                    }
                }
                __syncthreads();
            }
        }
    }
    uint4 *__restrict__ dst = table + (uint64_t)L * E + ci.start;
    for (uint32_t i = t; i < n; i += blockDim.x) dst[i] = src[pos[i]];
}

// maxInterval == 0 (every delay is 0) or no events
__global__ __launch_bounds__(256) void k_stats_constant(uint64_t n, uint32_t E,
                                                        nmz_sched_stats *__restrict__ stats) {
    uint64_t s = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (s >= n) return;
    nmz_sched_stats st;
    stats_empty(st);
    if (E) {
        st.max_delay_ns = 0;
        st.argmax_event = 0;
    }
    stats[s] = st;
}

// full per-decision dump for the first n_dump seeds (parity / debugging path):
// plain FNV over seed bytes || hint bytes, independent of the table
__global__ __launch_bounds__(256) void k_replayable_dump(const uint32_t *__restrict__ soff,
                                                         const uint8_t *__restrict__ sbytes,
                                                         uint64_t n_dump, const uint32_t *__restrict__ hoff,
                                                         const uint8_t *__restrict__ hbytes, uint32_t E,
                                                         uint64_t m, int64_t *__restrict__ out) {
    uint64_t idx = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= n_dump * E) return;
    const uint64_t s = idx / E;
    const uint32_t e = (uint32_t)(idx % E);
    uint64_t h = FNV_OFFSET;
    for (uint32_t i = soff[s], end = soff[s + 1]; i < end; ++i) h = fnv_step(h, sbytes[i]);
    for (uint32_t i = hoff[e], end = hoff[e + 1]; i < end; ++i) h = fnv_step(h, hbytes[i]);
    out[idx] = m ? (int64_t)(h % m) : 0;
}

// the statistics kernels run this plan's sweeps: the wavelet trees, else the order queries (NMZ_REPLAY_OQ=0 sends
// m < 2^30 to the per-decision sweep instead)
static bool use_wt(const nmz_replayable_plan *p) {
    return p->wt.on && (replay_oq_enabled() || p->mod.kind != MOD_FAST);
}
static bool use_oq(const nmz_replayable_plan *p) {
    return p->oq.on && (replay_oq_enabled() || p->mod.kind != MOD_FAST);
}

// top-k on the wavelet-tree path: the seeds of the chunks at or above the k-th largest chunk maximum
// (NMZ_WT_TOPK=0: the general selection, for A/B runs)
static bool wt_topk_enabled() {
    static const bool on = [] {
        const char *e = ab_env("NMZ_WT_TOPK");
        return !(e && std::string(e) == "0");
    }();
    return on;
}

// Enqueue the sweep for device-resident seeds: stats for every seed, by the first kernel family that applies --
// constant, wavelet trees, order queries, per-decision.
// Seeds: the CSR d_soff / d_sbytes, or (d_soff == nullptr) the decimal strings of dec_lo .. dec_lo + S - 1, or a
// prepared set `pre` (bucketed already at the statistics kernels' granularity).
static int replayable_stats(nmz_replayable_plan *p, hipStream_t st, const uint32_t *d_soff,
                            const uint8_t *d_sbytes, uint64_t S, nmz_sched_stats *d_stats, uint64_t dec_lo = 0,
                            void *wt_topk_scratch = nullptr, const nmz_replayable_seeds *pre = nullptr) {
    if (S == 0) return NMZ_OK;
    const uint32_t E = p->n_events;
    if (E == 0 || p->mod.kind == MOD_ZERO) {
        hipLaunchKernelGGL(k_stats_constant, dim3(ceil_div(S, 256)), dim3(256), 0, st, S, E, d_stats);
        NMZ_HIP(hipGetLastError());
        return NMZ_OK;
    }
    const bool wt = use_wt(p), stats_kernel = wt || use_oq(p);
    SeedScratch sc;
    if (pre && stats_kernel) {
        sc = pre->sc;
    } else {
        NMZ_CHECK(S <= p->max_seeds, "more seeds than the plan was created for");
        sc = carve_seed_scratch(p->seed_scratch.ptr, p->max_seeds);
        if (pre) {  // a per-decision sweep of prepared seeds: their hashes and row counts, bucketed there
            NMZ_HIP(hipMemcpyAsync(sc.b.hist, pre->hist, bucket_hist_u32(S) * sizeof(uint32_t),
                                   hipMemcpyDeviceToDevice, st));
            sc.h0 = pre->sc.h0;
        } else {
            NMZ_TRY(seed_prefix_launch(st, d_soff, d_sbytes, dec_lo, S, sc.h0, sc.b.hist));
        }
        if (stats_kernel) NMZ_TRY(bucket_seeds_counted(st, sc.h0, S, OQ_WG, sc.b, sc.counter));
    }
    if (wt) return wt_sweep(p->wt, p->ctx, st, sc.b, p->d_table, E, p->mod, d_stats, S, wt_topk_scratch);
    if (stats_kernel) return oq_sweep(p->oq, p->ctx, st, sc.b, p->d_table, E, p->mod, d_stats);
    return pd_sweep(p, st, sc, S, d_stats);
}

// Optional top-k (k > 0): by (sum_delay desc, seed asc) over the seeds' stats (n_fault = 0), seed =
// seed0 + seed index. (A merge kernel with the first selection level fused in measured 66 us against
// 21 + 29 us for k_replayable_merge + k_topk_chunk at 2^20 seeds, so the levels stay separate.)
static int replayable_run_on(nmz_replayable_plan *p, hipStream_t st, const uint32_t *d_soff, const uint8_t *d_sbytes,
                             uint64_t S, nmz_sched_stats *d_stats, uint64_t seed0, uint32_t k, nmz_topk_entry *d_topk,
                             uint64_t dec_lo, const nmz_replayable_seeds *pre);

static int replayable_run(nmz_replayable_plan *p, hipStream_t st, const uint32_t *d_soff, const uint8_t *d_sbytes,
                          uint64_t S, nmz_sched_stats *d_stats, uint64_t seed0 = 0, uint32_t k = 0,
                          nmz_topk_entry *d_topk = nullptr, uint64_t dec_lo = 0,
                          const nmz_replayable_seeds *pre = nullptr) {
    nmz_replayable_plan::Use *u = nullptr;
    for (auto &x : p->uses)
        if (x.st == st) u = &x;
    if (!u) {  // the plan's first sweep on this stream: the stream waits for the build (a no-op once it is done)
        hipEvent_t ev;
        NMZ_HIP(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        p->uses.push_back({st, ev});
        u = &p->uses.back();
        if (p->built && st != p->ctx->stream) NMZ_HIP(hipStreamWaitEvent(st, p->built, 0));
    }
    const int rc = replayable_run_on(p, st, d_soff, d_sbytes, S, d_stats, seed0, k, d_topk, dec_lo, pre);
    NMZ_HIP(hipEventRecord(u->ev, st));
    return rc;
}

// the plan's build and every sweep enqueued with it are done: its pooled buffers may go back to the context
static void plan_wait_uses(nmz_replayable_plan *p) {
    for (auto &u : p->uses) {
        (void)hipEventSynchronize(u.ev);
        (void)hipEventDestroy(u.ev);
    }
    p->uses.clear();
    if (p->built) {
        (void)hipEventSynchronize(p->built);
        (void)hipEventDestroy(p->built);
        p->built = nullptr;
    } else {
        (void)hipStreamSynchronize(p->ctx->stream);
    }
}

static int replayable_run_on(nmz_replayable_plan *p, hipStream_t st, const uint32_t *d_soff, const uint8_t *d_sbytes,
                             uint64_t S, nmz_sched_stats *d_stats, uint64_t seed0, uint32_t k, nmz_topk_entry *d_topk,
                             uint64_t dec_lo, const nmz_replayable_seeds *pre) {
    NMZ_CHECK(k <= 256, "top-k supports k <= 256");
    NMZ_CHECK(k == 0 || d_topk, "d_topk is NULL");
    // the wavelet-tree sweep's own top-k (k <= 64): the sweep leaves one record per 64-seed chunk in the plan's
    // scratch (O(S / 64) records, every one written by the sweep: nothing to reset), and one selection kernel takes
    // the k best from the chunks at or above the k-th largest chunk maximum, reading their sums from d_stats. Larger
    // k, other sweeps and NMZ_WT_TOPK=0 take the general selection over the stats
    const bool fused = k && k <= 64 && S > 0 && use_wt(p) && wt_topk_enabled();
    if (fused) NMZ_TRY(p->wt_topk.ensure(wt_topk_scratch_bytes(S)));
    NMZ_TRY(replayable_stats(p, st, d_soff, d_sbytes, S, d_stats, dec_lo, fused ? p->wt_topk.ptr : nullptr, pre));
    if (fused) {  // the bucketing of the sweep that ran (the prepared set's, or this plan's own)
        const Buckets b = pre ? pre->sc.b : carve_seed_scratch(p->seed_scratch.ptr, p->max_seeds).b;
        return wt_topk(st, p->wt_topk.ptr, b.offset, b.sorted_idx, d_stats, S, seed0, k, d_topk);
    }
    if (k) {
        NMZ_TRY(p->topk_lists.ensure(topk_scratch_entries(S, k) * sizeof(nmz_topk_entry)));
        NMZ_TRY(topk_select(st, d_stats, S, seed0, k, p->topk_lists.as<nmz_topk_entry>(), d_topk));
    }
    return NMZ_OK;
}

// The one place a plan is released, finished or half built. The caller holds the plan's context: the buffers go
// back to the context's pool, where the next plan may write them at once, so wait for the work still reading them
// -- the build and the sweeps on every stream the plan was used on (a plan whose build failed has no uses and no
// `built` event: plan_wait_uses then synchronises the context's stream, the build's)
static void plan_destroy_locked(nmz_replayable_plan *plan) {
    plan_wait_uses(plan);
    for (DevBuf *b : plan->buffers()) b->release();
    delete plan;
}

static int plan_create(nmz_ctx *ctx, const uint32_t *hint_off, const uint8_t *hint_bytes, uint32_t E,
                       int64_t max_interval, uint64_t max_seeds, nmz_replayable_plan **out, bool async = false) {
    NMZ_CHECK(ctx && out, "NULL argument");
    NMZ_CHECK(E == 0 || hint_off, "hint_off is NULL");
    *out = nullptr;
    auto *p = new nmz_replayable_plan();
    p->ctx = ctx;
    for (DevBuf *b : p->buffers()) b->pool = &ctx->pool;
    p->n_events = E;
    p->max_interval = max_interval;
    p->mod = make_mod((uint64_t)max_interval);  // uint64(r.MaxInterval), replayablepolicy.go:110
    p->max_seeds = max_seeds;
    hipStream_t st = ctx->stream;

    // length classes (stable, so original order is kept inside a class): a counting sort by hint length (a
    // comparison sort of 4,096 hints was ~100 us of the plan's host time)
    std::vector<uint32_t> perm(E);
    uint32_t maxlen = 0;
    for (uint32_t e = 0; e < E; ++e) maxlen = std::max(maxlen, hint_off[e + 1] - hint_off[e]);
    if (maxlen > 4 * (uint64_t)E + 4096) {  // a few very long hints: a comparison sort
        std::iota(perm.begin(), perm.end(), 0u);
        std::stable_sort(perm.begin(), perm.end(), [&](uint32_t a, uint32_t b) {
            return hint_off[a + 1] - hint_off[a] < hint_off[b + 1] - hint_off[b];
        });
    } else {
        std::vector<uint32_t> pos((size_t)maxlen + 2, 0);
        for (uint32_t e = 0; e < E; ++e) ++pos[hint_off[e + 1] - hint_off[e] + 1];
        for (size_t l = 1; l < pos.size(); ++l) pos[l] += pos[l - 1];
        for (uint32_t e = 0; e < E; ++e) perm[pos[hint_off[e + 1] - hint_off[e]]++] = e;
    }
    std::vector<ClassInfo> cls;  // runs of equal length in the length-sorted order (P^len once per class)
    for (uint32_t i = 0, prev = 0; i < E; ++i) {
        const uint32_t e = perm[i];
        const uint32_t len = hint_off[e + 1] - hint_off[e];
        if (cls.empty() || len != prev) {
            cls.push_back(ClassInfo{fnv_pow(len), i, 0});
            prev = len;
        }
        cls.back().count++;
    }
    p->n_classes = (uint32_t)cls.size();
    const uint64_t nbytes = E ? hint_off[E] : 0;

    // the wavelet-tree plan kernel computes and C-sorts the table itself when every class fits one of its segments:
    // its segment descriptors and zeroed row sums go up with the plan's inputs, and it zeroes the seed scratch's
    // counters itself -- one upload and one launch. (NMZ_WT_FUSED=0 takes the separate kernels always: parity tests
    // and A/B runs.)
    std::vector<WtClass> woc;
    const bool fused = E && !(ab_env("NMZ_WT_FUSED") && atoi(ab_env("NMZ_WT_FUSED")) == 0) &&
                       wt_layout(p->wt, ctx, E, cls.data(), (uint32_t)cls.size(), p->mod, true, woc);
    // the small inputs first (one contiguous region, packed in the context's pinned staging at the same offsets:
    // one asynchronous upload), then the table
    uint32_t *d_perm;
    WtClass *d_wcls = nullptr;
    unsigned long long *d_rowsum = nullptr;
    ScratchLayout lay;
    lay.add(&p->d_classes, cls.size() + 1).add(&d_perm, E + 1).add(&p->d_hoff, E + 1).add(&p->d_hbytes, nbytes + 1);
    if (fused) lay.add(&d_wcls, woc.size()).add(&d_rowsum, 256);
    lay.add(&p->d_table, (size_t)256 * E + 1);
    int rc = lay.bind(p->plan_mem);
    SeedScratch sc0{};
    const bool seeds = E && p->mod.kind != MOD_ZERO;
    if (rc == NMZ_OK && seeds) {
        rc = seed_scratch_bind(p->seed_scratch, max_seeds, sc0);
        if (rc == NMZ_OK) {  // the work-item counter starts at zero (k_bucket_scatter re-zeroes it)
            if (!fused && hipMemsetAsync(sc0.counter, 0, 4 * sizeof(uint32_t), st) != hipSuccess)
                rc = fail(NMZ_EHIP, "hipMemsetAsync of the seed scratch failed");
        }
    }
    // a failed build: the plan goes the way every plan does (no uses, no `built` event yet: the wait is for st)
    auto cleanup = [&](int code) {
        plan_destroy_locked(p);
        return code;
    };
    if (rc != NMZ_OK) return cleanup(rc);
    uint32_t *d_hoff = p->d_hoff;
    uint8_t *d_hbytes = p->d_hbytes;
    const size_t in_bytes = (size_t)(reinterpret_cast<char *>(p->d_table) - static_cast<char *>(p->plan_mem.ptr));
    if (E) {
        HostPin &pin = ctx->pin[0];
        if (pin.ensure(in_bytes) != NMZ_OK) return cleanup(NMZ_ENOMEM);
        {
            char *h = static_cast<char *>(pin.ptr);
            auto at = [&](const void *d) { return h + (static_cast<const char *>(d) - static_cast<char *>(p->plan_mem.ptr)); };
            std::memcpy(at(p->d_classes), cls.data(), cls.size() * sizeof(ClassInfo));
            std::memcpy(at(d_perm), perm.data(), (size_t)E * 4);
            std::memcpy(at(d_hoff), hint_off, (size_t)(E + 1) * 4);
            if (nbytes) std::memcpy(at(d_hbytes), hint_bytes, nbytes);
            if (fused) {
                std::memcpy(at(d_wcls), woc.data(), woc.size() * sizeof(WtClass));
                std::memset(at(d_rowsum), 0, 256 * 8);
            }
        }
        if (hipMemcpyAsync(p->plan_mem.ptr, pin.ptr, in_bytes, hipMemcpyHostToDevice, st) || pin.mark(st))
            return cleanup(fail(NMZ_EHIP, "plan upload failed"));
        if (fused) {
            const WtPlanHints hz{d_hoff, d_hbytes, d_perm, p->d_table,
                                 nullptr, 0u, seeds ? sc0.counter : nullptr, seeds ? 4u : 0u};
            const int wrc = wt_launch(p->wt, p->d_table, E, p->mod, st, &hz, d_wcls, d_rowsum, !async);
            if (wrc != NMZ_OK) return cleanup(wrc);
        }
        if (!p->wt.on) {
            // unsorted table into scratch (the context's, grow-only: no free, so no device sync), then the
            // per-(L, class) C sort into place
            uint4 *d_tmp;
            ScratchLayout tmp_lay;
            const int trc = tmp_lay.add(&d_tmp, (size_t)256 * E).bind(ctx->buf[SLOT_PLAN_TMP]);
            if (trc != NMZ_OK) return cleanup(trc);
            hipLaunchKernelGGL(k_replayable_table, dim3(E), dim3(256), 0, st, d_hoff, d_hbytes, d_perm, E, p->mod.m,
                               p->mod.m32ok ? 1 : 0, d_tmp);
            uint32_t max_class = 0;
            for (const ClassInfo &c : cls) max_class = std::max(max_class, c.count);
            bool bad = false;
            if (max_class <= SEG_SORT_MAX) {  // LDS sort per segment
                hipLaunchKernelGGL(k_replayable_table_segsort, dim3(p->n_classes, 256), dim3(1024), 0, st,
                                   d_tmp, p->d_classes, E, p->d_table);
                // no sync when the order-query images follow: oq_build synchronises after its kernels
                bad = hipGetLastError() != hipSuccess ||
                      (!p->mod.m32ok && hipStreamSynchronize(st) != hipSuccess);
            } else if (max_class <= 16384) {  // O(n^2) rank sort on the device
                hipLaunchKernelGGL(k_replayable_table_sort, dim3(ceil_div(E, 256), 256), dim3(256), 0, st,
                                   d_tmp, p->d_classes, p->n_classes, E, p->d_table);
                bad = hipGetLastError() != hipSuccess || hipStreamSynchronize(st) != hipSuccess;
            } else {  // very large classes: sort the segments on the host
                std::vector<uint4> h((size_t)256 * E);
                bad = hipGetLastError() != hipSuccess ||
                      hipMemcpyAsync(h.data(), d_tmp, h.size() * sizeof(uint4), hipMemcpyDeviceToHost, st) !=
                          hipSuccess ||
                      hipStreamSynchronize(st) != hipSuccess;
                if (!bad) {
                    auto key = [](const uint4 &q) { return ((uint64_t)q.y << 32) | q.x; };
                    for (uint32_t L = 0; L < 256; ++L)
                        for (const ClassInfo &c : cls)
                            std::stable_sort(h.begin() + (size_t)L * E + c.start,
                                             h.begin() + (size_t)L * E + c.start + c.count,
                                             [&](const uint4 &a, const uint4 &b) { return key(a) < key(b); });
                    bad = hipMemcpyAsync(p->d_table, h.data(), h.size() * sizeof(uint4), hipMemcpyHostToDevice, st) !=
                              hipSuccess ||
                          hipStreamSynchronize(st) != hipSuccess;
                }
            }
            if (bad)
                return cleanup(fail(NMZ_EHIP, "plan table kernel failed"));
            // wavelet-tree images (the default sweep when they fit), else the order-query images
            int orc = wt_build(p->wt, ctx, p->d_table, E, cls.data(), (uint32_t)cls.size(), p->mod, st);
            if (orc != NMZ_OK) return cleanup(orc);
            if (!p->wt.on) orc = oq_build(p->oq, p->d_table, E, p->mod, cls, st);
            if (orc != NMZ_OK) return cleanup(orc);
        }
        // the plan is complete before it is returned (sweeps may run on any stream), or, from the asynchronous
        // entry point with the wavelet-tree plan kernel, enqueued: sweeps on other streams wait for `built`
        if (!p->oq.on && !p->wt.on && hipStreamSynchronize(st) != hipSuccess)
            return cleanup(fail(NMZ_EHIP, "plan build failed"));
    }
    if (hipEventCreateWithFlags(&p->built, hipEventDisableTiming) != hipSuccess) {
        p->built = nullptr;
        return cleanup(fail(NMZ_EHIP, "hipEventCreate failed"));
    }
    if (hipEventRecord(p->built, st) != hipSuccess) {
        (void)hipEventDestroy(p->built);  // never recorded: the wait must be for st itself
        p->built = nullptr;
        return cleanup(fail(NMZ_EHIP, "hipEventRecord failed"));
    }
    *out = p;
    return NMZ_OK;
}

}  // namespace nmz

using namespace nmz;

extern "C" {
int nmz_replayable_plan_create(nmz_ctx *ctx, const uint32_t *hint_off, const uint8_t *hint_bytes,
                               uint32_t n_events, int64_t max_interval_ns, uint64_t max_seeds,
                               nmz_replayable_plan **out) {
    NMZ_CHECK(ctx != nullptr, "ctx is NULL");
    CtxGuard g(ctx);
    NMZ_TRY(g.rc);
    return plan_create(ctx, hint_off, hint_bytes, n_events, max_interval_ns, max_seeds, out);
}

int nmz_replayable_plan_create_async(nmz_ctx *ctx, const uint32_t *hint_off, const uint8_t *hint_bytes,
                                     uint32_t n_events, int64_t max_interval_ns, uint64_t max_seeds,
                                     nmz_replayable_plan **out) {
    NMZ_CHECK(ctx != nullptr, "ctx is NULL");
    CtxGuard g(ctx);
    NMZ_TRY(g.rc);
    return plan_create(ctx, hint_off, hint_bytes, n_events, max_interval_ns, max_seeds, out, true);
}

int nmz_replayable_plan_destroy(nmz_replayable_plan *plan) {
    if (!plan) return NMZ_OK;
    {
        CtxGuard g(plan->ctx);
        plan_destroy_locked(plan);
    }
    return NMZ_OK;
}

int nmz_replayable_plan_kernel(const nmz_replayable_plan *plan) {
    if (!plan) return -1;
    return plan->wt.on ? 2 : plan->oq.on ? 1 : 0;
}

int nmz_replayable_plan_wt_info(const nmz_replayable_plan *plan, uint32_t *bb, uint32_t *planes,
                                uint64_t *image_bytes) {
    NMZ_CHECK(plan != nullptr, "plan is NULL");
    NMZ_CHECK(plan->wt.on, "the plan does not run the wavelet-tree kernel");
    if (bb) *bb = plan->wt.bb;
    if (planes) *planes = plan->wt.planes ? 1u : 0u;
    if (image_bytes) *image_bytes = (uint64_t)plan->wt.rb16 * 16u;
    return NMZ_OK;
}

int nmz_replayable_sweep_dev(nmz_replayable_plan *plan, const uint32_t *d_seed_off, const uint8_t *d_seed_bytes,
                             uint64_t n_seeds, nmz_sched_stats *d_stats, void *stream) {
    NMZ_CHECK(plan != nullptr, "plan is NULL");
    CtxGuard g(plan->ctx);
    NMZ_TRY(g.rc);
    hipStream_t st = stream ? (hipStream_t)stream : plan->ctx->stream;
    return replayable_run(plan, st, d_seed_off, d_seed_bytes, n_seeds, d_stats);
}

int nmz_replayable_sweep_topk_dev(nmz_replayable_plan *plan, const uint32_t *d_seed_off, const uint8_t *d_seed_bytes,
                                  uint64_t n_seeds, uint64_t seed0, uint32_t k, nmz_sched_stats *d_stats,
                                  nmz_topk_entry *d_topk, void *stream) {
    NMZ_CHECK(plan != nullptr, "plan is NULL");
    CtxGuard g(plan->ctx);
    NMZ_TRY(g.rc);
    hipStream_t st = stream ? (hipStream_t)stream : plan->ctx->stream;
    return replayable_run(plan, st, d_seed_off, d_seed_bytes, n_seeds, d_stats, seed0, k, d_topk);
}

int nmz_replayable_sweep_traces(nmz_ctx *ctx, uint32_t n_traces, const uint32_t *const *hint_off,
                                const uint8_t *const *hint_bytes, const uint32_t *n_events, int64_t max_interval_ns,
                                uint64_t seed_lo, uint64_t n_seeds, uint32_t k, nmz_topk_entry *topk) {
    NMZ_CHECK(ctx != nullptr, "ctx is NULL");
    NMZ_CHECK(n_traces == 0 || (hint_off && hint_bytes && n_events && topk), "NULL argument");
    NMZ_CHECK(k >= 1 && k <= 256, "1 <= k <= 256");
    NMZ_CHECK(n_seeds >= 1 && n_seeds < (1ULL << 32), "1 <= n_seeds < 2^32");
    CtxGuard g(ctx);
    NMZ_TRY(g.rc);
    if (n_traces == 0) return NMZ_OK;
    // the pipeline's resources: the private second context (the plans are built on its stream, so one trace's build
    // overlaps the previous trace's sweep), an event per trace in flight, the stats / top-k buffers per slot
    if (!ctx->helper) NMZ_TRY(nmz_open(ctx->device, &ctx->helper));
    for (int i = 0; i < 3; ++i)
        if (!ctx->sweep_ev[i]) NMZ_HIP(hipEventCreateWithFlags(&ctx->sweep_ev[i], hipEventDisableTiming));
    const uint64_t S = n_seeds;
    nmz_sched_stats *d_st[2];
    nmz_topk_entry *d_tk[2];
    ScratchLayout lay;
    lay.add(&d_st[0], S).add(&d_st[1], S).add(&d_tk[0], k).add(&d_tk[1], k);
    NMZ_TRY(lay.bind(ctx->buf[SLOT_KNN_LISTS_OR_TRACE_RINGS]));
    NMZ_TRY(ctx->tkpin.ensure(3 * (size_t)k * sizeof(nmz_topk_entry)));
    nmz_topk_entry *h_tk = static_cast<nmz_topk_entry *>(ctx->tkpin.ptr);
    nmz_replayable_seeds *ss = nullptr;
    NMZ_TRY(seeds_create_locked(ctx, nullptr, nullptr, S, seed_lo, &ss));
    std::vector<nmz_replayable_plan *> plans(n_traces, nullptr);
    hipStream_t st = ctx->stream;
    auto make = [&](uint32_t j) {
        return plan_create(ctx->helper, hint_off[j], hint_bytes[j], n_events[j], max_interval_ns, S, &plans[j], true);
    };
    auto finish = [&](uint32_t j) -> int {
        const int r = hipEventSynchronize(ctx->sweep_ev[j % 3]) == hipSuccess ? NMZ_OK
                                                                               : fail(NMZ_EHIP, "sweep failed");
        std::memcpy(topk + (size_t)j * k, h_tk + (size_t)(j % 3) * k, (size_t)k * sizeof(nmz_topk_entry));
        plan_destroy_locked(plans[j]);
        plans[j] = nullptr;
        return r;
    };
    // trace i + 2's build is enqueued while trace i sweeps; trace i's top-k comes back while trace i + 1 sweeps
    constexpr uint32_t AHEAD = 2;
    int rc = NMZ_OK;
    for (uint32_t j = 0; j < std::min(AHEAD, n_traces) && rc == NMZ_OK; ++j) rc = make(j);
    // The schedule: a two-stage pipeline -- every plan build on the helper context's stream, two traces ahead, every
    // sweep (+ top-k + its copy to the host) on ctx's stream behind the build it waits for, trace i - 1's top-k read
    // once trace i's sweep is enqueued: 0.153-0.155 ms per trace over 64 traces, against 0.154-0.156 for the
    // Python-driven stream in the same process (profiles/r05/traces_mode_ab). Measured slower there: each trace
    // sweeping on the stream its plan was built on, the next build but one behind that sweep (two streams, each
    // serial), 0.165; builds on the two contexts' streams and sweeps on two more, 0.185-0.188.
    for (uint32_t i = 0; i < n_traces && rc == NMZ_OK; ++i) {
        if (i + AHEAD < n_traces) rc = make(i + AHEAD);
        if (rc != NMZ_OK) break;
        rc = replayable_run(plans[i], st, nullptr, nullptr, S, d_st[i % 2], seed_lo, k, d_tk[i % 2], 0, ss);
        if (rc != NMZ_OK) break;
        if (hipMemcpyAsync(h_tk + (size_t)(i % 3) * k, d_tk[i % 2], (size_t)k * sizeof(nmz_topk_entry),
                           hipMemcpyDeviceToHost, st) != hipSuccess ||
            hipEventRecord(ctx->sweep_ev[i % 3], st) != hipSuccess) {
            rc = fail(NMZ_EHIP, "top-k copy failed");
            break;
        }
        // trace i stays in flight: waiting for it here would hold back the next plan builds
        if (i >= 1) rc = finish(i - 1);
        if (rc == NMZ_OK && i + 1 == n_traces) rc = finish(i);
    }
    // on an error: every plan still alive waits for its work and goes
    for (auto *p : plans)
        if (p) plan_destroy_locked(p);
    seeds_destroy_locked(ss);
    return rc;
}

int nmz_replayable_sweep_seeds_topk_dev(nmz_replayable_plan *plan, const nmz_replayable_seeds *seeds, uint64_t seed0,
                                        uint32_t k, nmz_sched_stats *d_stats, nmz_topk_entry *d_topk, void *stream) {
    NMZ_CHECK(plan != nullptr && seeds != nullptr, "NULL argument");
    NMZ_CHECK(seeds->ctx->device == plan->ctx->device, "the seed set and the plan are on different devices");
    CtxGuard g(plan->ctx);
    NMZ_TRY(g.rc);
    hipStream_t st = stream ? (hipStream_t)stream : plan->ctx->stream;
    return replayable_run(plan, st, nullptr, nullptr, seeds->S, d_stats, seed0, k, d_topk, 0, seeds);
}

int nmz_replayable_sweep_decimal_topk_dev(nmz_replayable_plan *plan, uint64_t seed_lo, uint64_t n_seeds, uint32_t k,
                                          nmz_sched_stats *d_stats, nmz_topk_entry *d_topk, void *stream) {
    NMZ_CHECK(plan != nullptr, "plan is NULL");
    NMZ_CHECK(n_seeds < (1ULL << 32), "at most 2^32-1 seeds per call");
    CtxGuard g(plan->ctx);
    NMZ_TRY(g.rc);
    hipStream_t st = stream ? (hipStream_t)stream : plan->ctx->stream;
    return replayable_run(plan, st, nullptr, nullptr, n_seeds, d_stats, seed_lo, k, d_topk, seed_lo);
}

int nmz_replayable_sweep(nmz_ctx *ctx, const uint32_t *seed_off, const uint8_t *seed_bytes, uint64_t n_seeds,
                         const uint32_t *hint_off, const uint8_t *hint_bytes, uint32_t n_events,
                         int64_t max_interval_ns, nmz_sched_stats *stats, int64_t *delays,
                         uint64_t n_dump_seeds, uint32_t k, nmz_topk_entry *topk) {
    NMZ_CHECK(ctx != nullptr, "ctx is NULL");
    NMZ_CHECK(n_seeds == 0 || seed_off, "seed_off is NULL");
    NMZ_CHECK(n_dump_seeds <= n_seeds, "n_dump_seeds > n_seeds");
    NMZ_CHECK(n_seeds < (1ULL << 32), "at most 2^32-1 seeds per call");
    CtxGuard g(ctx);
    NMZ_TRY(g.rc);
    hipStream_t st = ctx->stream;
    HostCall call(ctx);
    nmz_replayable_plan *plan = nullptr;
    NMZ_TRY(plan_create(ctx, hint_off, hint_bytes, n_events, max_interval_ns, n_seeds, &plan));
    call.own_plan<plan_destroy_locked>(plan);

    const uint64_t sbytes = n_seeds ? seed_off[n_seeds] : 0;
    const uint64_t tk_entries = topk_scratch_entries(n_seeds, k);
    uint32_t *d_soff;
    uint8_t *d_sb;
    nmz_sched_stats *d_stats;
    int64_t *d_dump;
    nmz_topk_entry *d_tk;
    ScratchLayout lay;
    lay.add(&d_soff, n_seeds + 1).add(&d_sb, sbytes + 1).add(&d_stats, n_seeds + 1);
    lay.add(&d_dump, n_dump_seeds * n_events + 1).add(&d_tk, tk_entries + k + 1);
    NMZ_TRY(lay.bind(ctx->buf[SLOT_SWEEP_HOST]));
    NMZ_TRY(upload_seeds(d_soff, d_sb, seed_off, seed_bytes, n_seeds, false, st));
    NMZ_TRY(replayable_run(plan, st, d_soff, d_sb, n_seeds, d_stats));
    if (n_dump_seeds && n_events) {
        hipLaunchKernelGGL(k_replayable_dump, dim3(ceil_div(n_dump_seeds * n_events, 256)), dim3(256), 0, st, d_soff,
                           d_sb, n_dump_seeds, plan->d_hoff, plan->d_hbytes, n_events, plan->mod.m, d_dump);
        NMZ_HIP(hipGetLastError());
    }
    if (k) NMZ_TRY(topk_select(st, d_stats, n_seeds, 0, k, d_tk, d_tk + tk_entries));
    if (stats) NMZ_TRY(copy_d2h(stats, d_stats, n_seeds, st));
    if (delays) NMZ_TRY(copy_d2h(delays, d_dump, n_dump_seeds * n_events, st));
    if (topk) NMZ_TRY(copy_d2h(topk, d_tk + tk_entries, k, st));
    return call.done();
}

// Online decisions on the calling host thread (Replayable.QueueEvent decides at enqueue, replayablepolicy.go:
// 116-126): FNV-1a 64 over seed || hint, then % uint64(maxInterval) -- k_replayable_dump's direct form.
int nmz_replayable_decide_host(const uint8_t *seed, uint32_t seed_len, const uint32_t *hint_off,
                               const uint8_t *hint_bytes, uint32_t n_events, int64_t max_interval_ns,
                               int64_t *delays) {
    if (n_events == 0) return NMZ_OK;
    NMZ_CHECK(hint_off && delays && (seed_len == 0 || seed), "NULL argument");
    const uint64_t m = (uint64_t)max_interval_ns;  // uint64(r.MaxInterval), replayablepolicy.go:110
    uint64_t h0 = FNV_OFFSET;
    for (uint32_t i = 0; i < seed_len; ++i) h0 = fnv_step(h0, seed[i]);
    for (uint32_t e = 0; e < n_events; ++e) {
        NMZ_CHECK(hint_off[e] <= hint_off[e + 1], "hint offsets must not decrease");
        NMZ_CHECK(hint_off[e] == hint_off[e + 1] || hint_bytes, "hint_bytes is NULL");
        if (m == 0) {  // :101-104
            delays[e] = 0;
            continue;
        }
        uint64_t h = h0;
        for (uint32_t b = hint_off[e]; b < hint_off[e + 1]; ++b) h = fnv_step(h, hint_bytes[b]);
        delays[e] = (int64_t)(h % m);
    }
    return NMZ_OK;
}

// Online decisions for one seed (Replayable.QueueEvent -> determineInterval, replayablepolicy.go:100-126): a batch
// of n pending events, one thread per event (k_replayable_dump: plain FNV over seed || hint, then % m). No plan:
// a batch of a few events needs no correction tables, only the launch.
int nmz_replayable_decide(nmz_ctx *ctx, const uint8_t *seed, uint32_t seed_len, const uint32_t *hint_off,
                          const uint8_t *hint_bytes, uint32_t n_events, int64_t max_interval_ns, int64_t *delays) {
    NMZ_CHECK(ctx != nullptr, "ctx is NULL");
    CtxGuard g(ctx);
    NMZ_TRY(g.rc);
    if (n_events == 0) return NMZ_OK;
    NMZ_CHECK(hint_off && delays && (seed_len == 0 || seed), "NULL argument");
    if (max_interval_ns == 0) {  // :101-104
        for (uint32_t e = 0; e < n_events; ++e) delays[e] = 0;
        return NMZ_OK;
    }
    for (uint32_t e = 0; e < n_events; ++e) NMZ_CHECK(hint_off[e] <= hint_off[e + 1], "hint offsets must not decrease");
    const uint32_t hbytes = hint_off[n_events];
    NMZ_CHECK(hbytes == 0 || hint_bytes, "hint_bytes is NULL");
    hipStream_t st = ctx->stream;
    const uint32_t soff[2] = {0, seed_len};
    HostCall call(ctx);
    uint32_t *d_soff, *d_hoff;
    // d_spare: the 256 bytes the old size arithmetic added at the end, kept so that the slot's size is unchanged;
    // it can go once sizes may change
    uint8_t *d_sb, *d_hb, *d_spare;
    int64_t *d_out;
    ScratchLayout lay;
    lay.add(&d_soff, 2).add(&d_sb, seed_len + 1).add(&d_hoff, n_events + 1).add(&d_hb, hbytes + 1);
    lay.add(&d_out, n_events).add(&d_spare, 256);
    NMZ_TRY(lay.bind(ctx->buf[SLOT_REPLAYABLE_DECIDE]));
    NMZ_TRY(copy_h2d(d_soff, soff, 2, st));
    NMZ_TRY(copy_h2d(d_sb, seed, seed_len, st));
    NMZ_TRY(copy_h2d(d_hoff, hint_off, (size_t)n_events + 1, st));
    NMZ_TRY(copy_h2d(d_hb, hint_bytes, hbytes, st));
    hipLaunchKernelGGL(k_replayable_dump, dim3(ceil_div(n_events, 256)), dim3(256), 0, st, d_soff, d_sb, (uint64_t)1,
                       d_hoff, d_hb, n_events, (uint64_t)max_interval_ns, d_out);
    NMZ_HIP(hipGetLastError());
    NMZ_TRY(copy_d2h(delays, d_out, n_events, st));
    return call.done();
}

}  // extern "C"
