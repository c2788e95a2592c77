// K3 -- replayable-policy seed sweep against event-order constraints (replayablepolicy.go:100-126).
//
// Replayable.QueueEvent releases every event at arrival + determineInterval(event), so a seed is a delivery
// order. For seed s and constraint c = {before, after, margin}:
//     release[s][e] = arrival[e] + FNV1a64(seed_s || hint_e) % uint64(MaxInterval)      (0 when MaxInterval == 0)
//     slack[s][c]   = release[s][after] - release[s][before] - margin
// and c is satisfied iff slack >= 0. Per seed: the mask of satisfied constraints, their number, the minimum slack
// and the first constraint attaining it; seeds are ranked by (n_satisfied desc, min_slack desc, seed asc), which is
// nmz_topk_entry's order under the mapping n_fault = n_satisfied, sum_delay_ns = min_slack, first_fault = argmin.
//
// Kernel: one lane per seed, seeds in their natural order. Only the 2 C events the constraints
// name are hashed, in the project's affine form FNV_hint(h0) = h0 * P^len + C_hint[h0 & 0xff]: the plan holds one
// 256-entry row of C per (constraint, side) -- 2 KiB, 16 cache lines -- and a lane gathers its entry by its own low
// byte. P^len and arrival[after] - arrival[before] - margin are wave-uniform scalar loads. No seed bucketing, so the
// statistics leave in seed order (coalesced) and the block's top-k (topk_block_select) sees the seeds' own indices.
// All per-seed state is scalar registers: no per-seed arrays, no scratch memory.
#include <algorithm>
#include <string>
#include <vector>

#include "nmz_common.h"
#include "nmz_internal.h"
#include "order_dev.h"
#include "replayable_plan.h"
#include "topk_dev.h"

namespace nmz {

constexpr int64_t ORDER_LIMIT = (int64_t)1 << 61;  // arrivals, margins and MaxInterval: every slack fits int64
constexpr uint32_t ORDER_MAX_CONSTRAINTS = 64;     // one bit each of sat_mask

// one constraint on the device (wave-uniform: scalar loads)
struct OrderCons {
    uint64_t pn_b, pn_a;  // P^len of the before / after hint
    int64_t base;         // arrival[after] - arrival[before] - margin
    uint64_t pad;
};
static_assert(sizeof(OrderCons) == 32, "OrderCons layout");

template <int KIND>
__global__ __launch_bounds__(TOPK_THREADS) void k_order_sweep(const uint64_t *__restrict__ h0, uint64_t n,
                                                               uint64_t seed0, const uint64_t *__restrict__ table,
                                                               const OrderCons *__restrict__ cons, uint32_t C,
                                                               uint64_t m, uint64_t mu, uint32_t k,
                                                               nmz_order_stats *__restrict__ stats,
                                                               nmz_topk_entry *__restrict__ lists) {
    __shared__ TopkShared sh;
    const uint64_t base = (uint64_t)blockIdx.x * TOPK_CHUNK;
    // seed r of this lane sits at chunk position r * TOPK_THREADS + t (topk_block_select's layout: coalesced)
    uint64_t h[TOPK_PER_THREAD], mask[TOPK_PER_THREAD];
    int64_t mn[TOPK_PER_THREAD];
    uint32_t ns[TOPK_PER_THREAD], am[TOPK_PER_THREAD];
#pragma unroll
    for (uint32_t r = 0; r < TOPK_PER_THREAD; ++r) {
        const uint64_t i = base + (uint64_t)r * TOPK_THREADS + threadIdx.x;
        h[r] = i < n ? h0[i] : 0;
        mask[r] = 0;
        mn[r] = INT64_MAX;
        ns[r] = 0;
        am[r] = 0;
    }
    for (uint32_t c = 0; c < C; ++c) {
        const OrderCons cc = cons[c];
        const uint64_t *__restrict__ tb = table + (size_t)c * 512;  // rows [before][256], [after][256]
#pragma unroll
        for (uint32_t r = 0; r < TOPK_PER_THREAD; ++r) {
            int64_t slack = cc.base;
            if (KIND != ORD_ZERO) {
                const uint32_t L = (uint32_t)h[r] & 0xffu;
                const uint64_t hb = h[r] * cc.pn_b + tb[L];
                const uint64_t ha = h[r] * cc.pn_a + tb[256 + L];
                slack += (int64_t)order_mod<KIND>(ha, m, mu) - (int64_t)order_mod<KIND>(hb, m, mu);
            }
            const bool sat = slack >= 0;
            mask[r] |= (uint64_t)sat << c;
            ns[r] += sat ? 1u : 0u;
            if (slack < mn[r]) {  // strict: the first constraint attaining the minimum
                mn[r] = slack;
                am[r] = c;
            }
        }
    }
    nmz_topk_entry e[TOPK_PER_THREAD];
#pragma unroll
    for (uint32_t r = 0; r < TOPK_PER_THREAD; ++r) {
        const uint64_t i = base + (uint64_t)r * TOPK_THREADS + threadIdx.x;
        e[r] = topk_sentinel();
        if (i < n) {
            if (stats) {
                nmz_order_stats s;
                s.sat_mask = mask[r];
                s.min_slack_ns = mn[r];
                s.n_satisfied = ns[r];
                s.argmin_constraint = am[r];
                stats[i] = s;
            }
            e[r].seed = seed0 + i;
            e[r].sum_delay_ns = mn[r];
            e[r].n_fault = ns[r];
            e[r].first_fault = am[r];
        }
    }
    if (k) topk_block_select<true>(e, k, lists + (uint64_t)blockIdx.x * k, sh);
}

// ---- host side -------------------------------------------------------------------------------------------------

// the limits of nmz_gpu.h, shared by the host decision and the plan
static int order_validate(const uint32_t *hint_off, const uint8_t *hint_bytes, uint32_t E, int64_t max_interval,
                          const int64_t *arrival, const nmz_order_constraint *cons, uint32_t C) {
    NMZ_CHECK(C >= 1 && C <= ORDER_MAX_CONSTRAINTS, "n_constraints must be in [1, 64]");
    NMZ_CHECK(cons != nullptr, "constraints is NULL");
    NMZ_CHECK(max_interval >= 0 && max_interval <= ORDER_LIMIT, "max_interval_ns must be in [0, 2^61]");
    NMZ_CHECK(E == 0 || (hint_off && arrival), "hint_off or arrival_ns is NULL");
    for (uint32_t c = 0; c < C; ++c) {
        const std::string at = "constraint " + std::to_string(c) + ": ";
        NMZ_CHECK(cons[c].before < E && cons[c].after < E, at + "event index out of range (n_events = " +
                                                                std::to_string(E) + ")");
        NMZ_CHECK(cons[c].before != cons[c].after, at + "before == after");
        NMZ_CHECK(cons[c].margin_ns >= 1 && cons[c].margin_ns <= ORDER_LIMIT, at + "margin_ns must be in [1, 2^61]");
    }
    for (uint32_t e = 0; e < E; ++e) {
        NMZ_CHECK(arrival[e] >= 0 && arrival[e] <= ORDER_LIMIT,
                  "arrival_ns[" + std::to_string(e) + "] must be in [0, 2^61]");
        NMZ_CHECK(hint_off[e] <= hint_off[e + 1], "hint offsets must not decrease");
        NMZ_CHECK(hint_off[e] == hint_off[e + 1] || hint_bytes, "hint_bytes is NULL");
    }
    return NMZ_OK;
}

}  // namespace nmz

struct nmz_replayable_order_plan {
    nmz_ctx *ctx = nullptr;
    uint32_t n_constraints = 0;
    int kind = 0;
    uint64_t m = 0, mu = 0;
    uint64_t max_seeds = 0;
    nmz::DevBuf mem;    // the tables, the constraints, the seeds' prefix hashes and their bucket counts
    nmz::DevBuf lists;  // per-block top-k lists and their merge scratch
    uint64_t *d_table = nullptr;  // [C][2][256] the hints' additive corrections by FNV low byte
    nmz::OrderCons *d_cons = nullptr;
    uint64_t *d_h0 = nullptr;
    uint32_t *d_rows = nullptr;
    // the streams the plan's sweeps were enqueued on, each with an event after its latest sweep (destroy waits)
    struct Use {
        hipStream_t st;
        hipEvent_t ev;
    };
    std::vector<Use> uses;
};

namespace nmz {

static void order_plan_destroy_locked(nmz_replayable_order_plan *p) {
    for (auto &u : p->uses) {
        (void)hipEventSynchronize(u.ev);
        (void)hipEventDestroy(u.ev);
    }
    p->mem.release();
    p->lists.release();
    delete p;
}

static int order_plan_create_locked(nmz_ctx *ctx, const uint32_t *hint_off, const uint8_t *hint_bytes, uint32_t E,
                                    int64_t max_interval, const int64_t *arrival, const nmz_order_constraint *cons,
                                    uint32_t C, uint64_t max_seeds, nmz_replayable_order_plan **out) {
    NMZ_TRY(order_validate(hint_off, hint_bytes, E, max_interval, arrival, cons, C));
    NMZ_CHECK(max_seeds < (1ULL << 32), "at most 2^32-1 seeds per sweep");
    // host build: 2 C hints x 256 low bytes (at most 32,768 short hashes)
    std::vector<uint64_t> table((size_t)C * 512);
    std::vector<OrderCons> oc(C);
    for (uint32_t c = 0; c < C; ++c) {
        const uint32_t ev[2] = {cons[c].before, cons[c].after};
        for (int side = 0; side < 2; ++side) {
            const uint32_t b0 = hint_off[ev[side]], b1 = hint_off[ev[side] + 1];
            const uint64_t pn = fnv_pow(b1 - b0);
            for (uint32_t L = 0; L < 256; ++L) {
                uint64_t h = L;
                for (uint32_t i = b0; i < b1; ++i) h = fnv_step(h, hint_bytes[i]);
                table[(size_t)c * 512 + side * 256 + L] = h - (uint64_t)L * pn;
            }
            (side ? oc[c].pn_a : oc[c].pn_b) = pn;
        }
        oc[c].base = arrival[cons[c].after] - arrival[cons[c].before] - cons[c].margin_ns;
        oc[c].pad = 0;
    }
    auto *p = new nmz_replayable_order_plan();
    p->ctx = ctx;
    p->mem.pool = &ctx->pool;
    p->lists.pool = &ctx->pool;
    p->n_constraints = C;
    p->m = (uint64_t)max_interval;  // uint64(r.MaxInterval), replayablepolicy.go:110
    p->kind = order_kind(p->m);
    p->mu = order_mu(p->m);
    p->max_seeds = max_seeds;
    const size_t ns = max_seeds ? max_seeds : 1;
    ScratchLayout lay;
    lay.add(&p->d_table, table.size()).add(&p->d_cons, C).add(&p->d_h0, ns).add(&p->d_rows, bucket_hist_u32(ns));
    int rc = lay.bind(p->mem);
    if (rc != NMZ_OK) {
        delete p;
        return rc;
    }
    hipStream_t st = ctx->stream;
    hipError_t e = hipMemcpyAsync(p->d_table, table.data(), table.size() * 8, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(p->d_cons, oc.data(), C * sizeof(OrderCons), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);  // the host arrays go out of scope; sweeps may take any stream
    if (e != hipSuccess) {
        (void)hipStreamSynchronize(st);
        p->mem.release();
        delete p;
        return fail(NMZ_EHIP, std::string("order plan upload: ") + hipGetErrorString(e));
    }
    *out = p;
    return NMZ_OK;
}

// enqueue one sweep: seeds = the device CSR, or (d_soff == nullptr) the decimal strings of dec_lo .. dec_lo + S - 1;
// top-k .seed = seed0 + the seed's index
static int order_run(nmz_replayable_order_plan *p, hipStream_t st, const uint32_t *d_soff, const uint8_t *d_sbytes,
                     uint64_t dec_lo, uint64_t S, uint64_t seed0, uint32_t k, nmz_order_stats *d_stats,
                     nmz_topk_entry *d_topk) {
    NMZ_CHECK(k <= 256, "top-k supports k <= 256");
    NMZ_CHECK(k == 0 || d_topk, "d_topk is NULL");
    NMZ_CHECK(S <= p->max_seeds, "more seeds than the plan was created for");
    if (S == 0 && k == 0) return NMZ_OK;
    const uint64_t blocks = std::max<uint64_t>(1, (S + TOPK_CHUNK - 1) / TOPK_CHUNK);
    nmz_topk_entry *la = d_topk, *lb = nullptr;
    if (k && blocks > 1) {
        NMZ_TRY(p->lists.ensure(2 * blocks * k * sizeof(nmz_topk_entry)));
        la = p->lists.as<nmz_topk_entry>();
        lb = la + blocks * k;
    }
    nmz_replayable_order_plan::Use *u = nullptr;
    for (auto &x : p->uses)
        if (x.st == st) u = &x;
    if (!u) {
        hipEvent_t ev;
        NMZ_HIP(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        p->uses.push_back({st, ev});
        u = &p->uses.back();
    }
    int rc = seed_prefix_launch(st, d_soff, d_sbytes, dec_lo, S, p->d_h0, p->d_rows);
    if (rc == NMZ_OK) {
        KernelTimer kt(p->ctx, st, "order_sweep");
#define NMZ_K3(KIND)                                                                                               \
    hipLaunchKernelGGL(k_order_sweep<KIND>, dim3((unsigned)blocks), dim3(TOPK_THREADS), 0, st, p->d_h0, S, seed0,  \
                       p->d_table, p->d_cons, p->n_constraints, p->m, p->mu, k, d_stats, la)
        switch (p->kind) {
            case ORD_ZERO: NMZ_K3(ORD_ZERO); break;
            case ORD_SMALL: NMZ_K3(ORD_SMALL); break;
            case ORD_MID: NMZ_K3(ORD_MID); break;
            default: NMZ_K3(ORD_WIDE); break;
        }
#undef NMZ_K3
        if (hipGetLastError() != hipSuccess) rc = fail(NMZ_EHIP, "k_order_sweep launch failed");
    }
    if (rc == NMZ_OK && k && blocks > 1) rc = topk_merge_lists(st, la, lb, blocks, k, d_topk);
    NMZ_HIP(hipEventRecord(u->ev, st));
    return rc;
}

// the host-pointer sweeps: plan + upload + sweep + results, synchronous
static int order_sweep_host(nmz_ctx *ctx, const uint32_t *seed_off, const uint8_t *seed_bytes, uint64_t seed_lo,
                            uint64_t n_seeds, const uint32_t *hint_off, const uint8_t *hint_bytes, uint32_t n_events,
                            int64_t max_interval_ns, const int64_t *arrival_ns, const nmz_order_constraint *constraints,
                            uint32_t n_constraints, uint32_t k, nmz_order_stats *stats, nmz_topk_entry *topk,
                            bool decimal) {
    NMZ_CHECK(ctx != nullptr, "ctx is NULL");
    NMZ_CHECK(decimal || n_seeds == 0 || seed_off, "seed_off is NULL");
    NMZ_CHECK(n_seeds < (1ULL << 32), "at most 2^32-1 seeds per call");
    NMZ_CHECK(k <= 256, "top-k supports k <= 256");
    CtxGuard g(ctx);
    NMZ_TRY(g.rc);
    HostCall call(ctx);
    nmz_replayable_order_plan *plan = nullptr;
    NMZ_TRY(order_plan_create_locked(ctx, hint_off, hint_bytes, n_events, max_interval_ns, arrival_ns, constraints,
                                     n_constraints, n_seeds, &plan));
    call.own_plan<order_plan_destroy_locked>(plan);
    hipStream_t st = ctx->stream;
    const uint32_t kk = topk ? k : 0;
    uint64_t sbytes;
    NMZ_TRY(seed_csr_bytes(seed_off, seed_bytes, n_seeds, decimal, &sbytes));
    uint32_t *d_soff;
    uint8_t *d_sb;
    nmz_order_stats *d_stats;
    nmz_topk_entry *d_tk;
    ScratchLayout lay;
    lay.add(&d_soff, n_seeds + 1).add(&d_sb, sbytes + 1).add(&d_stats, n_seeds + 1).add(&d_tk, kk + 1);
    NMZ_TRY(lay.bind(ctx->buf[SLOT_SWEEP_HOST]));
    NMZ_TRY(upload_seeds(d_soff, d_sb, seed_off, seed_bytes, n_seeds, decimal, st));
    NMZ_TRY(order_run(plan, st, decimal ? nullptr : d_soff, d_sb, seed_lo, n_seeds, decimal ? seed_lo : 0, kk,
                      stats ? d_stats : nullptr, d_tk));
    if (stats) NMZ_TRY(copy_d2h(stats, d_stats, n_seeds, st));
    NMZ_TRY(copy_d2h(topk, d_tk, kk, st));
    return call.done();
}

}  // namespace nmz

using namespace nmz;

extern "C" {

// One seed on the calling thread (Replayable.QueueEvent's release times, replayablepolicy.go:100-126): plain FNV-1a
// over seed || hint and a u64 remainder, so it checks the kernel's affine tables and Barrett reductions
// independently.
int nmz_replayable_order_host(const uint8_t *seed, uint32_t seed_len, const uint32_t *hint_off,
                              const uint8_t *hint_bytes, uint32_t n_events, int64_t max_interval_ns,
                              const int64_t *arrival_ns, const nmz_order_constraint *constraints,
                              uint32_t n_constraints, nmz_order_stats *stats, int64_t *slack) {
    NMZ_CHECK(seed_len == 0 || seed, "seed is NULL");
    NMZ_TRY(order_validate(hint_off, hint_bytes, n_events, max_interval_ns, arrival_ns, constraints, n_constraints));
    const uint64_t m = (uint64_t)max_interval_ns;  // uint64(r.MaxInterval), replayablepolicy.go:110
    uint64_t h0 = FNV_OFFSET;
    for (uint32_t i = 0; i < seed_len; ++i) h0 = fnv_step(h0, seed[i]);
    auto delay = [&](uint32_t e) -> int64_t {
        if (m == 0) return 0;  // :101-104
        uint64_t h = h0;
        for (uint32_t b = hint_off[e]; b < hint_off[e + 1]; ++b) h = fnv_step(h, hint_bytes[b]);
        return (int64_t)(h % m);
    };
    nmz_order_stats s{0, INT64_MAX, 0, 0};
    for (uint32_t c = 0; c < n_constraints; ++c) {
        const nmz_order_constraint &k = constraints[c];
        const int64_t sl = (arrival_ns[k.after] + delay(k.after)) - (arrival_ns[k.before] + delay(k.before)) -
                           k.margin_ns;
        if (slack) slack[c] = sl;
        if (sl >= 0) {
            s.sat_mask |= 1ull << c;
            ++s.n_satisfied;
        }
        if (sl < s.min_slack_ns) {
            s.min_slack_ns = sl;
            s.argmin_constraint = c;
        }
    }
    if (stats) *stats = s;
    return NMZ_OK;
}

int nmz_replayable_order_plan_create(nmz_ctx *ctx, const uint32_t *hint_off, const uint8_t *hint_bytes,
                                     uint32_t n_events, int64_t max_interval_ns, const int64_t *arrival_ns,
                                     const nmz_order_constraint *constraints, uint32_t n_constraints,
                                     uint64_t max_seeds, nmz_replayable_order_plan **out) {
    NMZ_CHECK(ctx && out, "NULL argument");
    *out = nullptr;
    CtxGuard g(ctx);
    NMZ_TRY(g.rc);
    return order_plan_create_locked(ctx, hint_off, hint_bytes, n_events, max_interval_ns, arrival_ns, constraints,
                                    n_constraints, max_seeds, out);
}

int nmz_replayable_order_plan_destroy(nmz_replayable_order_plan *plan) {
    if (!plan) return NMZ_OK;
    CtxGuard g(plan->ctx);
    NMZ_TRY(g.rc);
    order_plan_destroy_locked(plan);
    return NMZ_OK;
}

int nmz_replayable_order_sweep_decimal_dev(nmz_replayable_order_plan *plan, uint64_t seed_lo, uint64_t n_seeds,
                                           uint32_t k, nmz_order_stats *d_stats, nmz_topk_entry *d_topk,
                                           void *stream) {
    NMZ_CHECK(plan != nullptr, "plan is NULL");
    CtxGuard g(plan->ctx);
    NMZ_TRY(g.rc);
    return order_run(plan, stream ? (hipStream_t)stream : plan->ctx->stream, nullptr, nullptr, seed_lo, n_seeds,
                     seed_lo, k, d_stats, d_topk);
}

int nmz_replayable_order_sweep_dev(nmz_replayable_order_plan *plan, const uint32_t *d_seed_off,
                                   const uint8_t *d_seed_bytes, uint64_t n_seeds, uint64_t seed0, uint32_t k,
                                   nmz_order_stats *d_stats, nmz_topk_entry *d_topk, void *stream) {
    NMZ_CHECK(plan != nullptr, "plan is NULL");
    NMZ_CHECK(n_seeds == 0 || d_seed_off, "d_seed_off is NULL");
    CtxGuard g(plan->ctx);
    NMZ_TRY(g.rc);
    return order_run(plan, stream ? (hipStream_t)stream : plan->ctx->stream, d_seed_off, d_seed_bytes, 0, n_seeds,
                     seed0, k, d_stats, d_topk);
}

int nmz_replayable_order_sweep(nmz_ctx *ctx, const uint32_t *seed_off, const uint8_t *seed_bytes, uint64_t n_seeds,
                               const uint32_t *hint_off, const uint8_t *hint_bytes, uint32_t n_events,
                               int64_t max_interval_ns, const int64_t *arrival_ns,
                               const nmz_order_constraint *constraints, uint32_t n_constraints, uint32_t k,
                               nmz_order_stats *stats, nmz_topk_entry *topk) {
    return order_sweep_host(ctx, seed_off, seed_bytes, 0, n_seeds, hint_off, hint_bytes, n_events, max_interval_ns,
                            arrival_ns, constraints, n_constraints, k, stats, topk, false);
}

int nmz_replayable_order_sweep_decimal(nmz_ctx *ctx, uint64_t seed_lo, uint64_t n_seeds, const uint32_t *hint_off,
                                       const uint8_t *hint_bytes, uint32_t n_events, int64_t max_interval_ns,
                                       const int64_t *arrival_ns, const nmz_order_constraint *constraints,
                                       uint32_t n_constraints, uint32_t k, nmz_order_stats *stats,
                                       nmz_topk_entry *topk) {
    return order_sweep_host(ctx, nullptr, nullptr, seed_lo, n_seeds, hint_off, hint_bytes, n_events, max_interval_ns,
                            arrival_ns, constraints, n_constraints, k, stats, topk, true);
}

}  // extern "C"
