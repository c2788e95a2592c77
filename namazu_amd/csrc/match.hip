// K7 -- match stored runs to the event universe: the pos[R][E] array the order contrast (K6) and the nearest-order
// sweep (K1t) take, made on the device (historystorage/naive/naive.go:235-257 walks the stored runs;
// historystorage/historystorage.go:45 GetStoredHistory hands each one out).
//
// The universe is sym[E] with arrival_ns[E]. The events carrying one symbol value are ordered by (arrival asc, event
// index asc); occurrence j of that order is "the j-th event with the symbol". Run r is the symbol slice
// run_sym[run_off[r] .. run_off[r + 1]). The i-th occurrence of a value in the run (counting from 0 in run order), at
// run position p, is matched to the i-th event with that value: pos[r][e] = p. Events without a matched occurrence
// keep NMZ_NONE; run elements whose value is not in the universe, and occurrences beyond the universe's count of
// the value, are ignored. namazu_amd/historystorage.py match_target is the same rule in numpy.
//
// The plan (host build, nmz_match_plan_create) holds usym[U] (the distinct symbols, ascending), start[U + 1] (each
// symbol's slice of the event list) and ev[E] (the events by (symbol, arrival, index)).
//
// k_match_runs: one workgroup per run, grid-striding over the runs; T threads and tiles of
// 4 T run elements, T in {64, 256, 1024} by the plan's E (mt_threads), so a small universe runs its -- usually
// short -- runs on one-wave workgroups, many to a CU. LDS: usym[U] (8 B), the staged output row[E] (4 B), the tile's
// keys[4 T] (4 B) and cur[U] (2 B): each symbol's cursor into ev[], start[u] at the head of a run, saturating at
// start[u + 1]. Per tile:
//   1. the run symbols by 16-byte loads (a tile starts on a 16-byte boundary of run_sym: the run is given one
//      virtual leading element where its first symbol is not aligned), each looked up by a 64-bit binary search of
//      usym -> key = u << 12 | index in tile (u = 4096: not in the universe, sorts last);
//   2. a bitonic sort of the keys in LDS over the next power of two of the tile's fill -- the keys are distinct, so
//      the network need not be stable: equal symbols end up adjacent, in run order;
//   3. sorted slot s: rank in its group = s - (first slot of the group, a binary search of the sorted keys); the
//      occurrence's event is ev[cur[u] + rank] if that is below start[u + 1]; its run position goes to the row;
//   4. behind a barrier the last slot of each group advances cur[u] (one writer per symbol, no atomics).
// The row is written out coalesced once per run (16 bytes per lane when the row is aligned) and reset on the way.
// No scratch; nothing is allocated per call.
#include <algorithm>
#include <string>
#include <vector>

#include "nmz_common.h"
#include "nmz_internal.h"

namespace nmz {

constexpr uint32_t MT_MAX_EVENTS = NMZ_DELIVERY_MAX_EVENTS;
constexpr uint32_t MT_IDX_BITS = 12;             // index in tile: tiles hold at most 4,096 elements
constexpr uint32_t MT_IDX_MASK = (1u << MT_IDX_BITS) - 1;
constexpr uint32_t MT_U_NONE = MT_MAX_EVENTS;    // dense id of "not in the universe": behind every symbol
constexpr uint32_t MT_PER_THREAD = 4;            // tile = 4 T
constexpr uint32_t MT_MAX_THREADS = 1024;
constexpr uint64_t MT_MAX_RUN = 0xFFFFFFFFull;   // run positions 0 .. 2^32 - 2 (NMZ_NONE stays free)
constexpr size_t MT_LDS_CU = 160 * 1024;
static_assert(MT_MAX_THREADS * MT_PER_THREAD == (1u << MT_IDX_BITS), "the largest tile fills the index bits");
static_assert(MT_MAX_EVENTS <= (1u << 12), "dense symbol ids and event indices fit 12 bits (+ the none id)");

struct MtArgs {
    const uint64_t *usym;   // [U] ascending
    const uint16_t *start;  // [U + 1]
    const uint16_t *ev;     // [E]
    uint32_t E, U;
    const uint64_t *run_off;  // [n_runs + 1]
    const uint64_t *run_sym;
    uint64_t n_runs;
    uint32_t *pos;  // [n_runs][E]
    uint32_t vec;   // rows are 16-byte aligned: E % 4 == 0 and pos is
};

// workgroup width for a universe of E events
static uint32_t mt_threads(uint32_t E) { return E <= 256 ? 64u : (E <= 1024 ? 256u : 1024u); }
static size_t mt_lds_bytes(uint32_t E, uint32_t U, uint32_t T) {
    return (size_t)((U + 1) & ~1u) * 8 + (size_t)((E + 3) & ~3u) * 4 + (size_t)T * MT_PER_THREAD * 4 +
           (((size_t)U * 2 + 3) & ~size_t(3));
}

// dense id of symbol s: 64-bit exact lower bound over usym[0 .. U), U >= 1
__device__ __forceinline__ uint32_t mt_lookup(const uint64_t *usym, uint32_t U, uint64_t s) {
    uint32_t lo = 0, n = U;
    while (n > 1) {
        const uint32_t half = n >> 1;
        lo = usym[lo + half] <= s ? lo + half : lo;
        n -= half;
    }
    return usym[lo] == s ? lo : MT_U_NONE;
}

__global__ __launch_bounds__(MT_MAX_THREADS) void k_match_runs(const MtArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint64_t mt_lds[];
    const uint32_t T = blockDim.x, tid = threadIdx.x, TILE = T * MT_PER_THREAD;
    const uint32_t E = a.E, U = a.U, E4 = (E + 3) & ~3u;
    uint64_t *usym = mt_lds;
    uint32_t *row = reinterpret_cast<uint32_t *>(usym + ((U + 1) & ~1u));
    uint32_t *keys = row + E4;
    uint16_t *cur = reinterpret_cast<uint16_t *>(keys + TILE);

    for (uint32_t i = tid; i < U; i += T) {
        usym[i] = a.usym[i];
        cur[i] = a.start[i];
    }
    for (uint32_t i = tid; i < E4; i += T) row[i] = NMZ_NONE;
    __syncthreads();

    for (uint64_t r = blockIdx.x; r < a.n_runs; r += gridDim.x) {
        const uint64_t lo = a.run_off[r], hi = a.run_off[r + 1];
        const uint64_t len = hi > lo ? min(hi - lo, MT_MAX_RUN) : 0;
        // one virtual leading element where the run's first symbol is not on a 16-byte boundary
        const uint32_t lead = (uint32_t)((reinterpret_cast<uintptr_t>(a.run_sym + lo) >> 3) & 1);
        const uint64_t *__restrict__ src = a.run_sym + lo - lead;
        const uint64_t vlen = len ? len + lead : 0;
        for (uint64_t vb = 0; vb < vlen; vb += TILE) {
            const uint32_t fill = (uint32_t)min((uint64_t)TILE, vlen - vb);
            uint32_t m = 2;  // the sorted span: a power of two covering the fill
            while (m < fill) m <<= 1;
            // 1. symbols -> keys
#pragma unroll
            for (uint32_t j = 0; j < MT_PER_THREAD / 2; ++j) {
                const uint32_t i0 = 2 * (tid + j * T);
                const uint64_t v0 = vb + i0;
                const bool ok0 = v0 >= lead && v0 < vlen, ok1 = v0 + 1 < vlen;  // v0 + 1 >= 1 >= lead
                uint64_t s0 = 0, s1 = 0;
                if (ok0 && ok1) {
                    const ulonglong2 q = *reinterpret_cast<const ulonglong2 *>(src + v0);
                    s0 = q.x;
                    s1 = q.y;
                } else {
                    if (ok0) s0 = src[v0];
                    if (ok1) s1 = src[v0 + 1];
                }
                const uint32_t u0 = ok0 ? mt_lookup(usym, U, s0) : MT_U_NONE;
                const uint32_t u1 = ok1 ? mt_lookup(usym, U, s1) : MT_U_NONE;
                keys[i0] = u0 << MT_IDX_BITS | i0;
                keys[i0 + 1] = u1 << MT_IDX_BITS | (i0 + 1);
            }
            __syncthreads();
            // 2. bitonic sort of keys[0 .. m), ascending
            for (uint32_t k = 2; k <= m; k <<= 1) {
                for (uint32_t j = k >> 1; j > 0; j >>= 1) {
                    for (uint32_t t = tid; t < (m >> 1); t += T) {
                        const uint32_t i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), p = i | j;
                        const uint32_t x = keys[i], y = keys[p];
                        if ((x > y) == ((i & k) == 0)) {
                            keys[i] = y;
                            keys[p] = x;
                        }
                    }
                    __syncthreads();
                }
            }
            // 3. ranks, events, the row
            uint32_t tail_u[MT_PER_THREAD], tail_c[MT_PER_THREAD];
#pragma unroll
            for (uint32_t j = 0; j < MT_PER_THREAD; ++j) {
                const uint32_t s = tid + j * T;
                tail_u[j] = MT_U_NONE;
                tail_c[j] = 0;
                if (s >= m) continue;
                const uint32_t key = keys[s], u = key >> MT_IDX_BITS;
                if (u >= U) continue;
                const uint32_t next = s + 1 < m ? keys[s + 1] >> MT_IDX_BITS : MT_U_NONE;
                // the group's first slot: the number of keys below u << 12 (the key at s is not, so head <= s < m)
                const uint32_t first = u << MT_IDX_BITS;
                uint32_t head = 0;
                for (uint32_t step = m >> 1; step; step >>= 1) head += keys[head + step - 1] < first ? step : 0u;
                const uint32_t lim = a.start[u + 1];
                const uint32_t slot = (uint32_t)cur[u] + (s - head);
                if (slot < lim) row[a.ev[slot]] = (uint32_t)(vb + (key & MT_IDX_MASK) - lead);
                if (next != u) {  // the group's last slot carries the cursor on
                    tail_u[j] = u;
                    tail_c[j] = min(slot + 1, lim);
                }
            }
            __syncthreads();
            // 4. one writer per symbol
#pragma unroll
            for (uint32_t j = 0; j < MT_PER_THREAD; ++j)
                if (tail_u[j] != MT_U_NONE) cur[tail_u[j]] = (uint16_t)tail_c[j];
            // the next tile's key writes follow the barrier above; its barriers order these cursor writes
        }
        __syncthreads();
        // the row out, reset behind it
        uint32_t *__restrict__ out = a.pos + r * E;
        if (a.vec) {
            uint4 *row4 = reinterpret_cast<uint4 *>(row);
            uint4 *out4 = reinterpret_cast<uint4 *>(out);
            for (uint32_t i = tid; i < (E >> 2); i += T) {
                out4[i] = row4[i];
                row4[i] = make_uint4(NMZ_NONE, NMZ_NONE, NMZ_NONE, NMZ_NONE);
            }
        } else {
            for (uint32_t i = tid; i < E; i += T) {
                out[i] = row[i];
                row[i] = NMZ_NONE;
            }
        }
        for (uint32_t i = tid; i < U; i += T) cur[i] = a.start[i];
        __syncthreads();
    }
}

}  // namespace nmz

struct nmz_match_plan {
    nmz_ctx *ctx = nullptr;
    uint32_t n_events = 0;
    uint32_t n_symbols = 0;
    nmz::DevBuf mem;  // usym, start, ev
    nmz::MtArgs args{};
    // the streams the plan's matches were enqueued on, each with an event after its latest one (destroy waits)
    struct Use {
        hipStream_t st;
        hipEvent_t ev;
    };
    std::vector<Use> uses;
};

namespace nmz {

// the universe's limits: no look at the arrays
static int match_universe(const uint64_t *sym, const int64_t *arrival, uint32_t E) {
    NMZ_CHECK(E >= 1 && E <= MT_MAX_EVENTS, "n_events must be in [1, 4096]");
    NMZ_CHECK(sym && arrival, "sym or arrival_ns is NULL");
    return NMZ_OK;
}

int match_validate(const uint64_t *sym, const int64_t *arrival, uint32_t E, const uint64_t *run_off,
                   const uint64_t *run_sym, uint64_t n_runs) {
    NMZ_TRY(match_universe(sym, arrival, E));
    NMZ_CHECK(n_runs <= (SIZE_MAX / sizeof(uint32_t)) / E, "n_runs * n_events does not fit the output");
    if (n_runs == 0) return NMZ_OK;
    NMZ_CHECK(run_off != nullptr, "run_off is NULL");
    NMZ_CHECK(run_off[0] == 0, "run_off[0] must be 0");
    for (uint64_t r = 0; r < n_runs; ++r) {
        NMZ_CHECK(run_off[r] <= run_off[r + 1], "run_off must be non-decreasing (run " + std::to_string(r) + ")");
        NMZ_CHECK(run_off[r + 1] - run_off[r] < MT_MAX_RUN,
                  "run " + std::to_string(r) + " has " + std::to_string(run_off[r + 1] - run_off[r]) +
                      " elements: at most 2^32 - 2");
    }
    NMZ_CHECK(run_off[n_runs] == 0 || run_sym, "run_sym is NULL");
    return NMZ_OK;
}

static void match_plan_destroy_locked(nmz_match_plan *p) {
    for (auto &u : p->uses) {
        (void)hipEventSynchronize(u.ev);
        (void)hipEventDestroy(u.ev);
    }
    p->mem.release();
    delete p;
}

// the universe has been checked (match_universe)
static int match_plan_create_locked(nmz_ctx *ctx, const uint64_t *sym, const int64_t *arrival, uint32_t E,
                                    nmz_match_plan **out) {
    // the events by (symbol, arrival, index): each symbol's slice is its occurrence order
    std::vector<uint16_t> ev(E);
    for (uint32_t e = 0; e < E; ++e) ev[e] = (uint16_t)e;
    std::sort(ev.begin(), ev.end(), [&](uint16_t x, uint16_t y) {
        if (sym[x] != sym[y]) return sym[x] < sym[y];
        if (arrival[x] != arrival[y]) return arrival[x] < arrival[y];
        return x < y;
    });
    std::vector<uint64_t> usym;
    std::vector<uint16_t> start;
    for (uint32_t i = 0; i < E; ++i)
        if (i == 0 || sym[ev[i]] != sym[ev[i - 1]]) {
            usym.push_back(sym[ev[i]]);
            start.push_back((uint16_t)i);
        }
    start.push_back((uint16_t)E);
    const uint32_t U = (uint32_t)usym.size();
    auto *p = new nmz_match_plan();
    p->ctx = ctx;
    p->mem.pool = &ctx->pool;
    p->n_events = E;
    p->n_symbols = U;
    uint64_t *d_usym;
    uint16_t *d_start, *d_ev;
    ScratchLayout lay;
    int rc = lay.add(&d_usym, U).add(&d_start, U + 1).add(&d_ev, E).bind(p->mem);
    if (rc != NMZ_OK) {
        delete p;
        return rc;
    }
    p->args = MtArgs{d_usym, d_start, d_ev, E, U, nullptr, nullptr, 0, nullptr, 0};
    hipStream_t st = ctx->stream;
    hipError_t e = hipMemcpyAsync(d_usym, usym.data(), (size_t)U * 8, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(d_start, start.data(), (size_t)(U + 1) * 2, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(d_ev, ev.data(), (size_t)E * 2, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);  // the host arrays go out of scope; matches may take any stream
    if (e != hipSuccess) {
        (void)hipStreamSynchronize(st);
        p->mem.release();
        delete p;
        return fail(NMZ_EHIP, std::string("match plan upload: ") + hipGetErrorString(e));
    }
    *out = p;
    return NMZ_OK;
}

static int match_enqueue(nmz_match_plan *p, hipStream_t st, const uint64_t *d_run_off, const uint64_t *d_run_sym,
                  uint64_t n_runs, uint32_t *d_pos) {
    const uint32_t E = p->n_events, U = p->n_symbols;
    NMZ_CHECK(n_runs <= (SIZE_MAX / sizeof(uint32_t)) / E, "n_runs * n_events does not fit the output");
    if (n_runs == 0) return NMZ_OK;
    NMZ_CHECK(d_run_off && d_pos, "d_run_off or d_pos is NULL");
    nmz_match_plan::Use *u = nullptr;
    for (auto &x : p->uses)
        if (x.st == st) u = &x;
    if (!u) {
        hipEvent_t ev;
        NMZ_HIP(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        p->uses.push_back({st, ev});
        u = &p->uses.back();
    }
    MtArgs a = p->args;
    a.run_off = d_run_off;
    a.run_sym = d_run_sym;
    a.n_runs = n_runs;
    a.pos = d_pos;
    a.vec = (E % 4 == 0 && (reinterpret_cast<uintptr_t>(d_pos) & 15) == 0) ? 1u : 0u;
    const uint32_t T = mt_threads(E);
    const size_t lds = mt_lds_bytes(E, U, T);
    // workgroups for every LDS and wave slot of the device
    const uint64_t per_cu = std::max<uint64_t>(1, std::min<uint64_t>(2048 / T, MT_LDS_CU / (lds + 512)));
    const unsigned blocks = (unsigned)std::min<uint64_t>(n_runs, (uint64_t)std::max(p->ctx->n_cu, 1) * per_cu);
    int rc = NMZ_OK;
    {
        KernelTimer kt(p->ctx, st, "match_runs");
        if (lds > 32 * 1024)  // beyond the default dynamic LDS of a launch; per device, cheap to repeat
            NMZ_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(k_match_runs),
                                        hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(k_match_runs, dim3(blocks), dim3(T), lds, st, a);
        if (hipGetLastError() != hipSuccess) rc = fail(NMZ_EHIP, "k_match_runs launch failed");
    }
    NMZ_HIP(hipEventRecord(u->ev, st));
    return rc;
}

int match_call(nmz_ctx *ctx, HostCall &call, const uint64_t *sym, const int64_t *arrival, uint32_t E,
               const uint64_t *run_off, const uint64_t *run_sym, uint64_t n_runs, uint32_t **d_pos) {
    nmz_match_plan *plan = nullptr;
    NMZ_TRY(match_plan_create_locked(ctx, sym, arrival, E, &plan));
    call.own_plan<match_plan_destroy_locked>(plan);
    uint64_t *d_off, *d_sym;
    ScratchLayout lay;
    lay.add(d_pos, (size_t)n_runs * E).add(&d_off, n_runs + 1).add(&d_sym, run_off[n_runs] + 1);
    NMZ_TRY(lay.bind(call.work));
    NMZ_TRY(upload_csr(d_off, d_sym, run_off, run_sym, n_runs, call.st));
    return match_enqueue(plan, call.st, d_off, d_sym, n_runs, *d_pos);
}

}  // namespace nmz

using namespace nmz;

extern "C" {

// One run on the calling thread (naive.go:235-257, historystorage.go:45 GetStoredHistory): plain loops by the
// definition -- the events in (arrival, index) order by one stable sort, then for each run element the first
// event with its symbol that no earlier element took. No symbol table, no cursor, nothing shared with the kernel.
int nmz_match_run_host(const uint64_t *sym, const int64_t *arrival_ns, uint32_t n_events, const uint64_t *run_sym,
                       uint64_t run_len, uint32_t *pos) {
    NMZ_TRY(match_universe(sym, arrival_ns, n_events));
    NMZ_CHECK(run_len < MT_MAX_RUN, "run has " + std::to_string(run_len) + " elements: at most 2^32 - 2");
    NMZ_CHECK(run_len == 0 || run_sym, "run_sym is NULL");
    NMZ_CHECK(pos != nullptr, "pos is NULL");
    std::vector<uint32_t> order(n_events);
    for (uint32_t e = 0; e < n_events; ++e) order[e] = e;
    std::stable_sort(order.begin(), order.end(),
                     [&](uint32_t x, uint32_t y) { return arrival_ns[x] < arrival_ns[y]; });
    for (uint32_t e = 0; e < n_events; ++e) pos[e] = NMZ_NONE;
    for (uint64_t p = 0; p < run_len; ++p)
        for (uint32_t i = 0; i < n_events; ++i) {
            const uint32_t e = order[i];
            if (sym[e] == run_sym[p] && pos[e] == NMZ_NONE) {
                pos[e] = (uint32_t)p;
                break;
            }
        }
    return NMZ_OK;
}

int nmz_match_plan_create(nmz_ctx *ctx, const uint64_t *sym, const int64_t *arrival_ns, uint32_t n_events,
                          nmz_match_plan **out) {
    NMZ_CHECK(ctx && out, "NULL argument");
    *out = nullptr;
    NMZ_TRY(match_universe(sym, arrival_ns, n_events));
    CtxGuard g(ctx);
    NMZ_TRY(g.rc);
    return match_plan_create_locked(ctx, sym, arrival_ns, n_events, out);
}

int nmz_match_plan_destroy(nmz_match_plan *plan) {
    if (!plan) return NMZ_OK;
    CtxGuard g(plan->ctx);
    NMZ_TRY(g.rc);
    match_plan_destroy_locked(plan);
    return NMZ_OK;
}

int nmz_match_plan_info(const nmz_match_plan *plan, uint32_t *n_events, uint32_t *n_symbols) {
    NMZ_CHECK(plan != nullptr, "plan is NULL");
    if (n_events) *n_events = plan->n_events;
    if (n_symbols) *n_symbols = plan->n_symbols;
    return NMZ_OK;
}

int nmz_match_runs_dev(nmz_match_plan *plan, const uint64_t *d_run_off, const uint64_t *d_run_sym, uint64_t n_runs,
                       uint32_t *d_pos, void *stream) {
    NMZ_CHECK(plan != nullptr, "plan is NULL");
    CtxGuard g(plan->ctx);
    NMZ_TRY(g.rc);
    return match_enqueue(plan, stream ? (hipStream_t)stream : plan->ctx->stream, d_run_off, d_run_sym, n_runs, d_pos);
}

int nmz_match_runs(nmz_ctx *ctx, const uint64_t *sym, const int64_t *arrival_ns, uint32_t n_events,
                   const uint64_t *run_off, const uint64_t *run_sym, uint64_t n_runs, uint32_t *pos) {
    // the arguments first: they are checked without a device
    NMZ_TRY(match_validate(sym, arrival_ns, n_events, run_off, run_sym, n_runs));
    if (n_runs == 0) return NMZ_OK;  // nothing to write: no device either
    NMZ_CHECK(pos != nullptr, "pos is NULL");
    NMZ_CHECK(ctx != nullptr, "ctx is NULL");
    CtxGuard g(ctx);
    NMZ_TRY(g.rc);
    HostCall call(ctx);
    uint32_t *d_pos = nullptr;
    NMZ_TRY(match_call(ctx, call, sym, arrival_ns, n_events, run_off, run_sym, n_runs, &d_pos));
    NMZ_TRY(copy_d2h(pos, d_pos, (size_t)n_runs * n_events, call.st));
    return call.done();
}

}  // extern "C"
