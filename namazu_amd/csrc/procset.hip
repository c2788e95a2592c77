// K5 -- ProcSetEvent decisions of the random policy (procPolicy: mild, extreme, dirichlet).
//
// Reference (randompolicy.go:300-304; mild.go:44-57; extreme.go:44-63; dirichlet.go:58-82): every ProcSetEvent gets
// a ProcSetSchedAction with one scheduling attribute per process of the set,
//   mild       nice_i = -20 + Int31n(40)
//   extreme    `prioritized` times mark slot Int31n(n); then a marked slot gets {RR, priority = Int31n(10)}
//   dirichlet  reset_i = Intn(999) < int(resetProbability * 1000.0)
// under the deterministic restatement: the generator of K2, the delay drawn first (no fault
// draw: a ProcSetEvent is not deferred), then the sub-policy's draws. One decision takes up to 513 generator outputs
// where K2 takes two, so the outputs come from the general closed form y_t (go_output, t < 607).
//
// Sweep kernel: K2's layout (one seed per lane, seeds bucketed by the low byte of their FNV prefix, so the per-event
// FNV correction is a scalar load; a persistent grid takes (unit, event chunk) items from a global counter). Inside
// one event the output index t is the same for every lane as long as no lane re-draws, so the power-table and cooked
// entries of y_t are scalar operands and the vector work is the modmuls, the reduction mod n and the accumulation.
// A lane whose draw is rejected (<= 2.4e-7 per draw; the delay draw of an arbitrary interval up to 1/2) recomputes the
// event with the general per-lane form (ps_decide), the code the host and the dump / decide kernel run.
// extreme keeps each lane's set of marked slots (<= 512 bits) in LDS.
#include <cstdio>
#include <cstring>

#include "nmz_common.h"
#include "nmz_internal.h"
#define NMZ_COOKED_TABLE d_cooked_procset  // this unit's copy of rngCooked (random_dev.h)
#include "random_dev.h"

namespace nmz {

constexpr uint32_t PS_MAX_PROCS = NMZ_PROCSET_MAX_PROCS;
constexpr uint32_t PS_MARK_WORDS = PS_MAX_PROCS / 32;
// linuxsched's policy numbers and flag
constexpr uint32_t PS_SCHED_NORMAL = 0, PS_SCHED_RR = 2, PS_SCHED_BATCH = 3, PS_SCHED_DEADLINE = 6;
constexpr uint32_t PS_SCHED_RESET_ON_FORK = 1;

__host__ __device__ constexpr uint32_t int31n_max(uint32_t n) { return 0x7fffffffu - (0x80000000u % n); }  // rand.go

// One event as the kernels take it: n processes, the target slot (or NMZ_NONE), and for extreme's Int31n(n) the
// Barrett factor floor(2^32 / n) (0: n is a power of two, Go's mask path) and the rejection bound.
struct PsEvent {
    uint32_t n, target, mu, maxv;
};
static_assert(sizeof(PsEvent) == 16, "PsEvent is loaded as one uint4");

static PsEvent make_ps_event(uint32_t n, uint32_t target) {
    PsEvent ev{n, target, 0, 0x7fffffffu};
    if (n & (n - 1)) {
        ev.mu = (uint32_t)((1ull << 32) / n);
        ev.maxv = int31n_max(n);
    }
    return ev;
}

struct PsOut {
    int64_t delay;
    int32_t score_sum, target_score;  // one event: |score| <= 20 per process, <= 512 processes
    uint32_t n_special, overflow;
};

struct PsRng {
    uint32_t s;
    int t;
    uint32_t ovf;
};

// Int31() of the next output; past output 606 the decision is marked (NMZ_ERANGE) and draws read as accepted zeros
__host__ __device__ inline uint32_t ps_next31(PsRng &r) {
    if (r.t >= gorand::LEN) {
        r.ovf = 1;
        return 0;
    }
    return (uint32_t)(go_output(r.s, r.t++) >> 32) & 0x7fffffffu;
}

// Rand.Int31n (rand.go, Go 1.10), n > 0: the mask for powers of two, otherwise rejection above int31n_max(n)
__host__ __device__ inline uint32_t ps_int31n(PsRng &r, uint32_t n) {
    uint32_t v = ps_next31(r);
    if ((n & (n - 1)) == 0) return v & (n - 1);
    const uint32_t maxv = int31n_max(n);
    while (v > maxv) v = ps_next31(r);
    return v % n;
}

struct NoAttrs {
    __host__ __device__ void operator()(uint32_t, uint32_t, int32_t, uint32_t, uint32_t) const {}
};
struct WriteAttrs {
    nmz_proc_attr *a;
    __host__ __device__ void operator()(uint32_t slot, uint32_t policy, int32_t nice, uint32_t priority,
                                        uint32_t flags) const {
        a[slot] = nmz_proc_attr{policy, nice, priority, flags};
    }
};
struct LocalMarks {
    uint32_t m[PS_MARK_WORDS];
    __host__ __device__ uint32_t &operator[](uint32_t w) { return m[w]; }
};

// The decision of one event in its general form: seed s, n processes, target slot; every draw through a per-decision
// output counter. Marks holds extreme's marked-slot set (word w = slots 32w .. 32w + 31); Attrs receives every slot.
template <class Marks, class Attrs>
__host__ __device__ inline PsOut ps_decide(uint32_t s, const ClassParams &cp, const nmz_procset_params &P, uint32_t n,
                                           uint32_t target, Marks &marks, const Attrs &attrs) {
    PsOut o{cp.min, 0, 0, 0, 0};
    PsRng r{s, 0, 0};
    if (cp.n) {  // the delay, as K2's decide()
        uint64_t v = go_output(s, r.t++) & MASK63;
        if (cp.mu) {
            while (v > cp.max_accept) {
                if (r.t >= gorand::LEN) {
                    r.ovf = 1;
                    break;
                }
                v = go_output(s, r.t++) & MASK63;
            }
            o.delay = (int64_t)mod_barrett(v, cp.n, cp.mu) + cp.min;
        } else {
            o.delay = (int64_t)(v & (cp.n - 1)) + cp.min;
        }
    }
    if (P.policy == NMZ_PROC_MILD) {
        const uint32_t pol = P.use_batch ? PS_SCHED_BATCH : PS_SCHED_NORMAL;
        for (uint32_t i = 0; i < n; ++i) {
            const int32_t nice = -20 + (int32_t)ps_int31n(r, 40);
            o.score_sum -= nice;
            o.n_special += nice < 0;
            if (i == target) o.target_score -= nice;
            attrs(i, pol, nice, 0, 0);
        }
    } else if (P.policy == NMZ_PROC_EXTREME) {
        for (uint32_t w = 0; w < (n + 31) / 32; ++w) marks[w] = 0;
        for (int32_t j = 0; j < P.prioritized; ++j) {
            const uint32_t slot = ps_int31n(r, n);
            marks[slot >> 5] |= 1u << (slot & 31);
        }
        for (uint32_t i = 0; i < n; ++i) {
            if ((marks[i >> 5] >> (i & 31)) & 1u) {
                const uint32_t pr = ps_int31n(r, 10);
                o.score_sum += 1 + pr;
                o.n_special += 1;
                if (i == target) o.target_score += 1 + pr;
                attrs(i, PS_SCHED_RR, 0, pr, 0);
            } else {
                attrs(i, PS_SCHED_BATCH, 0, 0, 0);
            }
        }
    } else {
        for (uint32_t i = 0; i < n; ++i) {
            const int32_t reset = (int32_t)ps_int31n(r, 999) < P.reset_threshold;
            o.score_sum += reset;
            o.n_special += reset;
            if (i == target) o.target_score += reset;
            attrs(i, reset ? PS_SCHED_NORMAL : PS_SCHED_DEADLINE, 0, 0, reset ? 0 : PS_SCHED_RESET_ON_FORK);
        }
    }
    o.overflow = r.ovf;
    return o;
}

// a lane's marked-slot set in LDS: word w of thread tid at [w][tid], so a wave's accesses to one word of its 64
// sets fall in 64 consecutive banks
struct LdsMarks {
    uint32_t *base;
    __device__ uint32_t &operator[](uint32_t w) { return base[w * 256]; }
};

__device__ __forceinline__ uint32_t hi31(uint64_t y) { return (uint32_t)(y >> 32) & 0x7fffffffu; }

// The sub-policy's draws of one event with a wave-uniform output index: outputs t0, t0 + 1, ... in the order of the
// general form, assuming every draw is accepted; rej is set when one is not (the caller then discards the result).
// At most t0 + 512 (mild, dirichlet) or t0 + 256 + 256 (extreme) <= 513 outputs, so the index never passes 606.
template <int POLICY>
__device__ __forceinline__ void ps_event_uniform(uint32_t s, uint32_t t0, const PsEvent &ev,
                                                 const nmz_procset_params &P, LdsMarks marks, int32_t &sum,
                                                 int32_t &tgt, uint32_t &nsp, bool &rej) {
    const uint32_t n = ev.n;
    if constexpr (POLICY == NMZ_PROC_MILD) {
        for (uint32_t i = 0; i < n; ++i) {
            const uint32_t v = hi31(go_output(s, (int)(t0 + i)));
            rej |= v > int31n_max(40);
            const int32_t sc = 20 - (int32_t)(v % 40u);  // -nice
            sum += sc;
            nsp += sc > 0;
            tgt += i == ev.target ? sc : 0;
        }
    } else if constexpr (POLICY == NMZ_PROC_DIRICHLET) {
        for (uint32_t i = 0; i < n; ++i) {
            const uint32_t v = hi31(go_output(s, (int)(t0 + i)));
            rej |= v > int31n_max(999);
            const int32_t reset = (int32_t)(v % 999u) < P.reset_threshold;
            sum += reset;
            tgt += i == ev.target ? reset : 0;
        }
        nsp += (uint32_t)sum;
    } else {
        const uint32_t nw = (n + 31) >> 5;
        for (uint32_t w = 0; w < nw; ++w) marks[w] = 0;
        const uint32_t np = P.prioritized > 0 ? (uint32_t)P.prioritized : 0u;
        for (uint32_t j = 0; j < np; ++j) {
            const uint32_t v = hi31(go_output(s, (int)(t0 + j)));
            uint32_t slot;
            if (ev.mu == 0) {
                slot = v & (n - 1);
            } else {
                rej |= v > ev.maxv;
                slot = v - umulhi32(v, ev.mu) * n;  // the quotient estimate is exact or one short: slot < 2n
                slot = slot >= n ? slot - n : slot;
            }
            marks[slot >> 5] |= 1u << (slot & 31);  // slot < n <= 512 whatever v is
        }
        // the marked slots draw their priorities in slot order: the j-th draw belongs to the j-th marked slot, so
        // the sum needs the first nsp draws and the target the draw whose rank is the marks below it
        const uint32_t tw = ev.target >> 5, tb = ev.target & 31;
        uint32_t cnt = 0, rank = NMZ_NONE;
        for (uint32_t w = 0; w < nw; ++w) {
            const uint32_t m = marks[w];
            if (ev.target != NMZ_NONE && w == tw && ((m >> tb) & 1u)) rank = cnt + __popc(m & ((1u << tb) - 1u));
            cnt += __popc(m);
        }
        nsp += cnt;
        const uint32_t t1 = t0 + np, lim = min(np, n);
        for (uint32_t j = 0; j < lim; ++j) {
            const bool act = j < cnt;
            if (__ballot(act) == 0) break;  // wave-uniform exit: j and the output index stay scalar
            const uint32_t v = hi31(go_output(s, (int)(t1 + j)));
            rej |= act && v > int31n_max(10);
            const int32_t sc = 1 + (int32_t)(v % 10u);
            sum += act ? sc : 0;
            tgt += j == rank ? sc : 0;
        }
    }
}

// Work item = (unit of <= 64 seeds sharing the low byte L, chunk of ec events), as K2. With one chunk an item writes
// its seeds' stats; with more, every field of the statistics is a sum (flags: an or), so the items add into zeroed
// stats with atomics and the result does not depend on their order.
template <int POLICY>
__global__ __launch_bounds__(256) void k_procset_sweep(const uint4 *__restrict__ units,
                                                       const uint32_t *__restrict__ n_units,
                                                       const uint64_t *__restrict__ sorted_h0,
                                                       const uint32_t *__restrict__ sorted_idx,
                                                       const uint4 *__restrict__ table,
                                                       const uint4 *__restrict__ events, uint32_t E, uint32_t ec,
                                                       uint32_t n_chunks, RandomKParams KP, nmz_procset_params P,
                                                       uint32_t *__restrict__ item_counter,
                                                       nmz_procset_stats *__restrict__ stats,
                                                       uint32_t *__restrict__ overflow) {
    __shared__ uint32_t lds_marks[PS_MARK_WORDS * 256];
    LdsMarks marks{lds_marks + threadIdx.x};
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t n_items = *n_units * n_chunks;
    const ClassParams c0 = KP.cls[0], c1 = KP.cls[1];
    for (;;) {
        uint32_t item = 0;
        if (lane == 0) item = atomicAdd(item_counter, 1u);
        item = __builtin_amdgcn_readfirstlane(__shfl(item, 0, 64));
        if (item >= n_items) break;
        const uint32_t unit = item / n_chunks, chunk = item - unit * n_chunks;
        const uint4 u = units[unit];
        const uint32_t L = __builtin_amdgcn_readfirstlane(u.x);
        const uint32_t start = __builtin_amdgcn_readfirstlane(u.y);
        const uint32_t cnt = __builtin_amdgcn_readfirstlane(u.z);
        const uint32_t e0 = chunk * ec, e1 = min(E, e0 + ec);
        const bool active = lane < cnt;
        const uint64_t h0 = active ? sorted_h0[start + lane] : 0;
        const uint64_t H = h0 * fnv_pow(8);
        const uint32_t Hm = (uint32_t)(H % gorand::M31);
        const uint4 *__restrict__ row = table + (uint64_t)L * E;

        uint64_t sum_delay = 0;
        int64_t score = 0, tscore = 0;
        uint32_t nsp = 0, ovf = 0;
        for (uint32_t e = e0; e < e1; ++e) {
            const uint32_t eu = __builtin_amdgcn_readfirstlane(e);
            const uint4 q = uniform4(row[eu]);
            const uint4 evq = uniform4(events[eu]);
            const PsEvent ev{evq.x, evq.y, evq.z, evq.w};
            const ClassParams &cp = (q.w & NMZ_EV_PRIORITIZED) ? c1 : c0;
            const uint32_t s = go_seed_from_table(H, Hm, q);
            int64_t delay = cp.min;
            bool rej = false;
            uint32_t t0 = 0;
            if (cp.n) {
                const uint64_t v = gorand::out0(s) & MASK63;
                t0 = 1;
                if (cp.mu) {
                    rej = v > cp.max_accept;
                    delay = (int64_t)mod_barrett(v, cp.n, cp.mu) + cp.min;
                } else {
                    delay = (int64_t)(v & (cp.n - 1)) + cp.min;
                }
            }
            int32_t es = 0, et = 0;
            uint32_t en = 0;
            ps_event_uniform<POLICY>(s, t0, ev, P, marks, es, et, en, rej);
            if (rej && active) {  // rare: this lane's output index left the wave's
                const PsOut o = ps_decide(s, cp, P, ev.n, ev.target, marks, NoAttrs{});
                delay = o.delay;
                es = o.score_sum;
                et = o.target_score;
                en = o.n_special;
                ovf |= o.overflow;
            }
            sum_delay += (uint64_t)delay;
            score += es;
            tscore += et;
            nsp += en;
        }
        if (!active) continue;
        nmz_procset_stats *o = stats + sorted_idx[start + lane];
        const uint32_t flags = ovf ? NMZ_STAT_RNG_OVERFLOW : 0u;
        if (ovf) atomicOr(overflow, 1u);
        if (n_chunks == 1) {
            *o = nmz_procset_stats{sum_delay, score, tscore, nsp, flags};
        } else {
            atomicAdd((unsigned long long *)&o->sum_delay_ns, (unsigned long long)sum_delay);
            atomicAdd((unsigned long long *)&o->score_sum, (unsigned long long)score);
            atomicAdd((unsigned long long *)&o->target_score, (unsigned long long)tscore);
            atomicAdd(&o->n_special, nsp);
            if (flags) atomicOr(&o->flags, flags);
        }
    }
}

// Every decision of seeds seed0 .. seed0 + n_seeds - 1 in full (the sweep's dump rows, and nmz_procset_decide with one
// seed): one thread per (seed, event), the direct form -- FNV over le64(seed) || le64(evhash), Go's seed reduction,
// ps_decide -- with no table. off[e] = the prefix sum of the events' process counts, total = their sum.
__global__ __launch_bounds__(256) void k_procset_decide(uint64_t seed0, uint64_t n_seeds,
                                                        const uint64_t *__restrict__ evhash,
                                                        const uint8_t *__restrict__ evclass,
                                                        const uint4 *__restrict__ events,
                                                        const uint64_t *__restrict__ off, uint64_t total, uint32_t E,
                                                        RandomKParams KP, nmz_procset_params P,
                                                        int64_t *__restrict__ delays,
                                                        nmz_proc_attr *__restrict__ attrs,
                                                        uint32_t *__restrict__ overflow) {
    const uint64_t idx = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= n_seeds * E) return;
    const uint64_t sidx = idx / E;
    const uint32_t e = (uint32_t)(idx % E);
    uint64_t h = seed_prefix(seed0 + sidx);
    const uint64_t eh = evhash[e];
#pragma unroll
    for (int i = 0; i < 8; ++i) h = fnv_step(h, (uint32_t)(eh >> (8 * i)) & 0xff);
    const uint32_t s = gorand::seed_reduce((int64_t)h);
    const uint4 evq = events[e];
    LocalMarks marks;
    const PsOut o = ps_decide(s, KP.cls[evclass[e] & NMZ_EV_PRIORITIZED], P, evq.x, NMZ_NONE, marks,
                              WriteAttrs{attrs + sidx * total + off[e]});
    delays[idx] = o.delay;
    if (o.overflow) atomicOr(overflow, 1u);
}

// top-k by target_score through the schedule top-k (topk.hip: n_fault desc, sum_delay desc, seed asc): the key is
// the score (negated for ascending order) in sum_delay's place, shifted so that the selection's coarse 48-bit key
// tells scores apart; |target_score| <= 20 * 2^32
constexpr int PS_KEY_SHIFT = 16;
__global__ __launch_bounds__(256) void k_procset_topk_keys(const nmz_procset_stats *__restrict__ stats, uint64_t n,
                                                           int descending, nmz_sched_stats *__restrict__ keys) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int64_t ts = stats[i].target_score;
    nmz_sched_stats k;
    stats_empty(k);
    k.sum_delay_ns = (uint64_t)((descending ? ts : -ts) * ((int64_t)1 << PS_KEY_SHIFT));
    keys[i] = k;
}

__global__ __launch_bounds__(256) void k_procset_topk_out(const nmz_topk_entry *__restrict__ in, uint32_t k,
                                                          int descending,
                                                          nmz_procset_topk_entry *__restrict__ out) {
    const uint32_t i = threadIdx.x;
    if (i >= k) return;
    const nmz_topk_entry x = in[i];
    nmz_procset_topk_entry y{x.seed, INT64_MIN};
    if (!(x.seed == UINT64_MAX && x.sum_delay_ns == INT64_MIN)) {  // not padding
        const int64_t ts = x.sum_delay_ns / ((int64_t)1 << PS_KEY_SHIFT);
        y.target_score = descending ? ts : -ts;
    }
    out[i] = y;
}

// The arguments every entry point shares: class bits, process counts, sub-policy parameters, target slots. Fills the
// events as the kernels take them and the prefix sums off[E + 1].
static int ps_inputs(const uint8_t *evclass, const uint32_t *n_procs, const uint32_t *target_slot, uint32_t E,
                     const nmz_procset_params *pp, std::vector<PsEvent> &events, std::vector<uint64_t> &off) {
    NMZ_CHECK(pp != nullptr, "procset params is NULL");
    NMZ_CHECK(pp->policy == NMZ_PROC_MILD || pp->policy == NMZ_PROC_EXTREME || pp->policy == NMZ_PROC_DIRICHLET,
              "bad procset policy");
    NMZ_CHECK(pp->prioritized <= (int32_t)NMZ_PROCSET_MAX_PRIORITIZED, "prioritized exceeds 256");
    NMZ_CHECK(E == 0 || (evclass && n_procs), "evclass/n_procs is NULL");
    events.resize(E);
    off.assign((size_t)E + 1, 0);
    for (uint32_t e = 0; e < E; ++e) {
        NMZ_CHECK((evclass[e] & ~NMZ_EV_PRIORITIZED) == 0,
                  "evclass of a ProcSetEvent may carry NMZ_EV_PRIORITIZED only (deferred=false: never faultable)");
        const uint32_t n = n_procs[e];
        NMZ_CHECK(n <= PS_MAX_PROCS, "n_procs exceeds 512");
        if (pp->policy == NMZ_PROC_EXTREME)
            NMZ_CHECK(n > 0 || pp->prioritized <= 0, "extreme: no process to prioritize (Int31n(0) panics)");
        if (pp->policy == NMZ_PROC_DIRICHLET) NMZ_CHECK(n > 0, "event has no process (dirichlet.go:43-45)");
        const uint32_t t = target_slot ? target_slot[e] : NMZ_NONE;
        NMZ_CHECK(t == NMZ_NONE || t < n, "target_slot is not a slot of its event");
        events[e] = make_ps_event(n, t);
        off[e + 1] = off[e] + n;
    }
    return NMZ_OK;
}

static int ps_sweep_launch(nmz_random_plan *plan, hipStream_t st, uint64_t seed0, uint64_t S, const uint4 *d_events,
                           const nmz_procset_params &pp, nmz_procset_stats *d_stats, uint32_t *d_ovf) {
    const uint32_t E = plan->n_events;
    Buckets b;
    uint32_t *d_counter;
    NMZ_TRY(random_bucket(plan, st, seed0, S, b, &d_counter));
    // enough work items for several rounds of the persistent grid's waves, by cutting the events into chunks of
    // at least 8 when the seeds alone give too few units
    const uint64_t max_units = S / 64 + 256, slots = (uint64_t)plan->ctx->n_cu * 32;
    uint32_t n_chunks = (uint32_t)std::min<uint64_t>((8 * slots + max_units - 1) / max_units, std::max(1u, E / 8));
    const uint32_t ec = (E + n_chunks - 1) / n_chunks;
    n_chunks = (E + ec - 1) / ec;
    if (n_chunks > 1) NMZ_HIP(hipMemsetAsync(d_stats, 0, S * sizeof(nmz_procset_stats), st));
    const unsigned grid = (unsigned)std::min<uint64_t>(plan->ctx->n_cu * 8ull, ceil_div(max_units * n_chunks, 4));
    KernelTimer kt(plan->ctx, st, "procset_sweep");
#define NMZ_PS_LAUNCH(POLICY)                                                                                    \
    hipLaunchKernelGGL(k_procset_sweep<POLICY>, dim3(grid), dim3(256), 0, st, b.units, b.n_units, b.sorted_h0,   \
                       b.sorted_idx, plan->d_table, d_events, E, ec, n_chunks, plan->kp, pp, d_counter, d_stats,  \
                       d_ovf)
    if (pp.policy == NMZ_PROC_MILD)
        NMZ_PS_LAUNCH(NMZ_PROC_MILD);
    else if (pp.policy == NMZ_PROC_EXTREME)
        NMZ_PS_LAUNCH(NMZ_PROC_EXTREME);
    else
        NMZ_PS_LAUNCH(NMZ_PROC_DIRICHLET);
#undef NMZ_PS_LAUNCH
    NMZ_HIP(hipGetLastError());
    return NMZ_OK;
}

// uploads the inputs of k_procset_decide and runs it for n_seeds seeds; the results stay on the device
struct PsDecideBufs {
    uint64_t *d_eh, *d_off;
    uint8_t *d_ec;
    uint4 *d_events;
    int64_t *d_del;
    nmz_proc_attr *d_attr;
    uint32_t *d_ovf;
};
// the fields of the decisions of n_seeds seeds over E events with `total` processes, appended to the call's layout
static void ps_decide_layout(ScratchLayout &lay, uint32_t E, uint64_t n_seeds, uint64_t total, PsDecideBufs &o) {
    lay.add(&o.d_eh, E + 1).add(&o.d_off, E + 1).add(&o.d_ec, E + 1).add(&o.d_events, E + 1);
    lay.add(&o.d_del, n_seeds * E + 1).add(&o.d_attr, n_seeds * total + 1).add(&o.d_ovf, 4);
}
static int ps_decide_launch(const PsDecideBufs &o, hipStream_t st, uint64_t seed0, uint64_t n_seeds,
                            const uint64_t *evhash, const uint8_t *evclass, const std::vector<PsEvent> &events,
                            const std::vector<uint64_t> &off, const RandomKParams &kp, const nmz_procset_params &pp) {
    const uint32_t E = (uint32_t)events.size();
    const uint64_t total = off[E];
    NMZ_HIP(hipMemsetAsync(o.d_ovf, 0, 4, st));
    NMZ_TRY(copy_h2d(o.d_eh, evhash, E, st));
    NMZ_TRY(copy_h2d(o.d_off, off.data(), E, st));
    NMZ_TRY(copy_h2d(o.d_ec, evclass, E, st));
    if (E == 0) return NMZ_OK;
    // a PsEvent is loaded as one uint4
    NMZ_HIP(hipMemcpyAsync(o.d_events, events.data(), (size_t)E * sizeof(PsEvent), hipMemcpyHostToDevice, st));
    if (n_seeds) {
        hipLaunchKernelGGL(k_procset_decide, dim3(ceil_div(n_seeds * E, 256)), dim3(256), 0, st, seed0, n_seeds,
                           o.d_eh, o.d_ec, o.d_events, o.d_off, total, E, kp, pp, o.d_del, o.d_attr, o.d_ovf);
        NMZ_HIP(hipGetLastError());
    }
    return NMZ_OK;
}

}  // namespace nmz

using namespace nmz;

extern "C" {

// loadProcConfig (randompolicy.go:230-270)
int nmz_procset_params_resolve(const char *proc_policy, int use_batch, int prioritized, double reset_probability,
                               nmz_procset_params *out) {
    NMZ_CHECK(out != nullptr, "out is NULL");
    const char *name = (proc_policy && *proc_policy) ? proc_policy : "mild";
    int policy;
    if (!std::strcmp(name, "mild"))
        policy = NMZ_PROC_MILD;
    else if (!std::strcmp(name, "extreme"))
        policy = NMZ_PROC_EXTREME;
    else if (!std::strcmp(name, "dirichlet"))
        policy = NMZ_PROC_DIRICHLET;
    else
        return fail(NMZ_EINVAL, std::string("bad procPolicy ") + name);
    if (policy == NMZ_PROC_DIRICHLET && !(reset_probability >= 0.0 && reset_probability <= 1.0)) {
        char m[96];
        std::snprintf(m, sizeof m, "bad procPolicyParam.resetProbability %f", reset_probability);
        return fail(NMZ_EINVAL, m);
    }
    NMZ_CHECK(prioritized <= (int)NMZ_PROCSET_MAX_PRIORITIZED,
              "procPolicyParam.prioritized exceeds 256 (a decision must fit 607 generator outputs)");
    out->policy = policy;
    out->use_batch = use_batch ? 1 : 0;
    out->prioritized = prioritized;
    // dirichlet.go:62 int(ResetProbability * 1000.0); the other policies never read it
    const bool in_range = reset_probability >= 0.0 && reset_probability <= 1.0;
    out->reset_threshold = in_range ? (int32_t)(reset_probability * 1000.0) : 0;
    return NMZ_OK;
}

// procPolicy.Action on the calling host thread (mild.go:30-57, extreme.go:30-63, dirichlet.go:38-82 under the
// DESIGN.md section 2 contract): FNV, seed reduction and ps_decide are the code the kernels run
int nmz_procset_decide_host(uint64_t seed, const uint64_t *evhash, const uint8_t *evclass, const uint32_t *n_procs,
                            uint32_t n_events, const nmz_random_params *random_params,
                            const nmz_procset_params *procset_params, int64_t *delays, nmz_proc_attr *attrs) {
    RandomKParams kp;
    NMZ_TRY(make_kparams(random_params, kp));
    std::vector<PsEvent> events;
    std::vector<uint64_t> off;
    NMZ_TRY(ps_inputs(evclass, n_procs, nullptr, n_events, procset_params, events, off));
    if (n_events == 0) return NMZ_OK;
    NMZ_CHECK(evhash && delays && (attrs || off[n_events] == 0), "NULL argument");
    const uint64_t h0 = seed_prefix(seed);
    for (uint32_t e = 0; e < n_events; ++e) {
        uint64_t h = h0;
        for (int i = 0; i < 8; ++i) h = fnv_step(h, (uint32_t)(evhash[e] >> (8 * i)) & 0xff);
        LocalMarks marks;
        const PsOut o = ps_decide(gorand::seed_reduce((int64_t)h), kp.cls[evclass[e] & NMZ_EV_PRIORITIZED],
                                  *procset_params, events[e].n, NMZ_NONE, marks, WriteAttrs{attrs + off[e]});
        if (o.overflow) return fail(NMZ_ERANGE, "a decision needed more than 607 Go rng outputs");
        delays[e] = o.delay;
    }
    return NMZ_OK;
}

int nmz_procset_decide(nmz_ctx *ctx, uint64_t seed, const uint64_t *evhash, const uint8_t *evclass,
                       const uint32_t *n_procs, uint32_t n_events, const nmz_random_params *random_params,
                       const nmz_procset_params *procset_params, int64_t *delays, nmz_proc_attr *attrs) {
    NMZ_CHECK(ctx != nullptr, "ctx is NULL");
    RandomKParams kp;
    NMZ_TRY(make_kparams(random_params, kp));
    std::vector<PsEvent> events;
    std::vector<uint64_t> off;
    NMZ_TRY(ps_inputs(evclass, n_procs, nullptr, n_events, procset_params, events, off));
    CtxGuard g(ctx);
    NMZ_TRY(g.rc);
    if (n_events == 0) return NMZ_OK;
    const uint64_t total = off[n_events];
    NMZ_CHECK(evhash && delays && (attrs || total == 0), "NULL argument");
    hipStream_t st = ctx->stream;
    uint32_t ovf = 0;
    HostCall call(ctx);
    PsDecideBufs d;
    ScratchLayout lay;
    ps_decide_layout(lay, n_events, 1, total, d);
    NMZ_TRY(lay.bind(ctx->buf[SLOT_RANDOM_PROCSET_DECIDE]));
    NMZ_TRY(ps_decide_launch(d, st, seed, 1, evhash, evclass, events, off, kp, *procset_params));
    NMZ_TRY(copy_d2h(delays, d.d_del, n_events, st));
    NMZ_TRY(copy_d2h(attrs, d.d_attr, total, st));
    NMZ_TRY(copy_d2h(&ovf, d.d_ovf, 1, st));
    NMZ_TRY(call.done());
    if (ovf) return fail(NMZ_ERANGE, "a decision needed more than 607 Go rng outputs");
    return NMZ_OK;
}

int nmz_procset_sweep(nmz_ctx *ctx, uint64_t seed0, uint64_t n_seeds, const uint64_t *evhash, const uint8_t *evclass,
                      const uint32_t *n_procs, const uint32_t *target_slot, uint32_t n_events,
                      const nmz_random_params *random_params, const nmz_procset_params *procset_params,
                      nmz_procset_stats *stats, int64_t *delays, nmz_proc_attr *attrs, uint64_t n_dump_seeds,
                      uint32_t k, int descending, nmz_procset_topk_entry *topk) {
    NMZ_CHECK(ctx != nullptr, "ctx is NULL");
    NMZ_CHECK(n_dump_seeds <= n_seeds, "n_dump_seeds > n_seeds");
    NMZ_CHECK(n_seeds < (1ULL << 32), "at most 2^32-1 seeds per call");
    NMZ_CHECK(k <= 256, "top-k supports k <= 256");
    std::vector<PsEvent> events;
    std::vector<uint64_t> off;
    NMZ_TRY(ps_inputs(evclass, n_procs, target_slot, n_events, procset_params, events, off));
    NMZ_CHECK(n_events == 0 || evhash, "evhash is NULL");
    CtxGuard g(ctx);
    NMZ_TRY(g.rc);
    hipStream_t st = ctx->stream;
    uint32_t ovf = 0;
    HostCall call(ctx);
    nmz_random_plan *plan = nullptr;
    NMZ_TRY(random_plan_create(ctx, evhash, evclass, n_events, random_params, n_seeds, &plan));
    call.own_plan<random_plan_free>(plan);
    const uint64_t total = off[n_events];
    const uint64_t tk_entries = topk_scratch_entries(n_seeds, k);
    nmz_procset_stats *d_stats;
    nmz_sched_stats *d_keys;
    nmz_topk_entry *d_tk;
    nmz_procset_topk_entry *d_out;
    PsDecideBufs d;
    ScratchLayout lay;
    lay.add(&d_stats, n_seeds + 1).add(&d_keys, n_seeds + 1).add(&d_tk, tk_entries + k + 1).add(&d_out, k + 1);
    ps_decide_layout(lay, n_events, n_dump_seeds, total, d);
    NMZ_TRY(lay.bind(ctx->buf[SLOT_RANDOM_PROCSET_SWEEP]));
    // the events and, for the dump rows, every decision of the first n_dump_seeds seeds in full
    NMZ_TRY(ps_decide_launch(d, st, seed0, n_dump_seeds, evhash, evclass, events, off, plan->kp, *procset_params));
    if (n_seeds) {
        if (n_events)
            NMZ_TRY(ps_sweep_launch(plan, st, seed0, n_seeds, d.d_events, *procset_params, d_stats, d.d_ovf));
        else  // no events: every sum is empty
            NMZ_HIP(hipMemsetAsync(d_stats, 0, n_seeds * sizeof(nmz_procset_stats), st));
    }
    if (k) {
        if (n_seeds)
            hipLaunchKernelGGL(k_procset_topk_keys, dim3(ceil_div(n_seeds, 256)), dim3(256), 0, st, d_stats, n_seeds,
                               descending, d_keys);
        NMZ_TRY(topk_select(st, d_keys, n_seeds, seed0, k, d_tk, d_tk + tk_entries));
        hipLaunchKernelGGL(k_procset_topk_out, dim3(1), dim3(256), 0, st, d_tk + tk_entries, k, descending, d_out);
        NMZ_HIP(hipGetLastError());
    }
    if (stats) NMZ_TRY(copy_d2h(stats, d_stats, n_seeds, st));
    if (delays) NMZ_TRY(copy_d2h(delays, d.d_del, n_dump_seeds * n_events, st));
    if (attrs) NMZ_TRY(copy_d2h(attrs, d.d_attr, n_dump_seeds * total, st));
    if (topk) NMZ_TRY(copy_d2h(topk, d_out, k, st));
    NMZ_TRY(copy_d2h(&ovf, d.d_ovf, 1, st));
    NMZ_TRY(call.done());
    if (ovf) return fail(NMZ_ERANGE, "a decision needed more than 607 Go rng outputs");
    return NMZ_OK;
}

}  // extern "C"
