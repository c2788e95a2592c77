// Shared host/device definitions for libnmz_gpu.so (gfx950 only).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/nmz_gpu.h"
#include "scratch_layout.h"

// ---------------------------------------------------------------------------
// error plumbing (thread-local message, int status codes of nmz_gpu.h)
// ---------------------------------------------------------------------------
namespace nmz {

void set_error(const std::string &msg);
int fail(int code, const std::string &msg);

#define NMZ_HIP(call)                                                                   \
    do {                                                                                \
        hipError_t e_ = (call);                                                         \
        if (e_ != hipSuccess)                                                           \
            return ::nmz::fail(NMZ_EHIP, std::string(#call) + ": " + hipGetErrorString(e_)); \
    } while (0)

#define NMZ_CHECK(cond, msg)                                                            \
    do {                                                                                \
        if (!(cond)) return ::nmz::fail(NMZ_EINVAL, (msg));                             \
    } while (0)

#define NMZ_TRY(expr)                                                                   \
    do {                                                                                \
        int rc_ = (expr);                                                               \
        if (rc_ != NMZ_OK) return rc_;                                                  \
    } while (0)

// Grow-only device scratch buffer owned by a context. With a pool (a plan's buffers: the context's list of
// free buffers), release() hands the memory back to the pool and ensure() reuses a pooled buffer before it
// allocates, so creating and destroying plans does not hipMalloc / hipFree (hipFree synchronises the device).
struct DevBuf {
    void *ptr = nullptr;
    size_t cap = 0;
    std::vector<DevBuf> *pool = nullptr;
    uint64_t gen = 0;  // bumped whenever ensure() hands out a different allocation (its contents are then undefined)
    // a context slot's name and in-use mark (ScratchLayout::bind sets it for the layout's lifetime and refuses a
    // marked slot); plan-owned and pool-backed buffers have no name and are never marked
    const char *slot = nullptr;
    bool busy = false;
    int ensure(size_t bytes);
    void release();
    template <typename T>
    T *as() const { return static_cast<T *>(ptr); }
};

// Grow-only pinned host staging owned by a context: a plan's inputs are packed here and reach the device in one
// asynchronous copy (a pageable hipMemcpyAsync stages through a driver buffer and returns only when that is done).
// The copy reading it is marked with an event (mark); ensure() waits for it before the buffer is packed again,
// so a build that returns before its upload finished (nmz_replayable_plan_create_async) is safe.
struct HostPin {
    void *ptr = nullptr;
    size_t cap = 0;
    hipEvent_t busy = nullptr;  // recorded after the last copy out of the buffer
    int ensure(size_t bytes);   // waits for that copy, then grows (a power of two of at least 1 MiB)
    int mark(hipStream_t st);
    void release();
};

// ---------------------------------------------------------------------------
// The context's scratch slots (nmz_ctx::buf). One enumerator per role. Two roles share a slot only where they can
// never be live in the same call; a slot bound twice in one call is refused by ScratchLayout::bind (NMZ_EINVAL).
// SLOT_TOPK alone is sized by a plain ensure() (one field plus a spare 256 bytes, which no layout's rounding gives)
// and so never carries the in-use mark.
// Live together, so their slots must stay distinct:
//   * SLOT_CONTRAST_HOST (nmz_order_contrast_runs), SLOT_CONTRAST_RUN (contrast_run) and match_call's pool buffer
//     (HostCall::work)
//   * SLOT_TARGET_DELIVERY_HOST (the delivery host form), SLOT_DELIVERY_CLASSES, SLOT_CLASSES (classes_launch)
//     and the rank-key table (nmz_ctx::rank_keys)
//   * SLOT_KNN_LISTS_OR_TRACE_RINGS (nmz_ed_plan_query_knn), SLOT_ED_QUERY_FORM (ed_query_bv) and its spill into
//     ed_query_generic_launch (SLOT_ED_QUERY_GENERIC)
// ---------------------------------------------------------------------------
#define NMZ_SLOTS(X)                                                                                                  \
    /* the order sweep's and the replayable sweep's host forms: each is one synchronous call holding the context */   \
    X(SLOT_SWEEP_HOST)                                                                                                \
    /* nmz_random_sweep and nmz_procset_sweep: host forms, one synchronous call each */                               \
    X(SLOT_RANDOM_PROCSET_SWEEP)                                                                                      \
    X(SLOT_ED_KNN_HOST)      /* nmz_ed_allpairs_knn: the lists and their ids and distances */                         \
    X(SLOT_ED_KNN)           /* ed_knn_run's generic fallback: a chunk of pairs, distances, DP rows */                \
    X(SLOT_ED_PAIRS_HOST)    /* nmz_ed_pairs */                                                                       \
    X(SLOT_TOPK)             /* nmz_topk_select_dev */                                                                \
    X(SLOT_CLASSES)          /* classes_launch: sort keys and payloads */                                             \
    X(SLOT_UNIQUE_HOST)      /* nmz_trace_signatures / nmz_unique_traces host forms */                                \
    X(SLOT_REPLAYABLE_DECIDE) /* nmz_replayable_decide */                                                             \
    /* nmz_random_decide and nmz_procset_decide: host forms, one synchronous call each */                             \
    X(SLOT_RANDOM_PROCSET_DECIDE)                                                                                     \
    X(SLOT_PLAN_TMP)         /* replayable plan creation: the wide-table build's temporary */                         \
    /* ed_query's ids and the replayable traces sweep's result rings: an ed plan query never runs inside a sweep */   \
    X(SLOT_KNN_LISTS_OR_TRACE_RINGS)                                                                                  \
    X(SLOT_FNV_BATCH)        /* nmz_fnv1a64_batch */                                                                  \
    /* ed_query_bv, ed_query_wide or ed_query_generic: the plan's kind picks one of them per call */                  \
    X(SLOT_ED_QUERY_FORM)                                                                                             \
    X(SLOT_ED_QUERY_GENERIC) /* ed_query_generic_launch, also as ed_query_bv's spill */                               \
    /* the target and the delivery sweeps' host forms: each is one synchronous call holding the context */            \
    X(SLOT_TARGET_DELIVERY_HOST)                                                                                      \
    X(SLOT_DELIVERY_CLASSES) /* delivery_classes_locked: signatures and best gaps */                                  \
    X(SLOT_CONTRAST_RUN)     /* contrast_run: the run order, the merged list, the per-workgroup lists */              \
    /* nmz_order_contrast and nmz_order_contrast_runs: host forms, one synchronous call each */                       \
    X(SLOT_CONTRAST_HOST)                                                                                             \
    X(SLOT_PO_SCAN)          /* po_project_enqueue: the temporary of the offsets' scan */
enum Slot : int {
#define X(name) name,
    NMZ_SLOTS(X)
#undef X
    SLOT_COUNT
};
constexpr const char *SLOT_NAMES[SLOT_COUNT] = {
#define X(name) #name,
    NMZ_SLOTS(X)
#undef X
};

}  // namespace nmz

// Optional HIP-event timing of the dominant kernels (bench.py reads it).
struct NmzTiming {
    bool enabled = false;
    bool spans_only = false;  // NMZ_TIMING_SPANS: span slots, no events
    std::map<std::string, std::vector<std::pair<hipEvent_t, hipEvent_t>>> events;
    std::vector<hipEvent_t> pool;
    // in-kernel execution spans: slot = {max ~start, max end} of wall_clock64() over the launch's workgroups
    unsigned long long *span_dev = nullptr;
    uint32_t span_next = 0;
    std::map<std::string, std::vector<uint32_t>> spans;
};
constexpr uint32_t NMZ_SPAN_SLOTS = 4096;

struct nmz_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    std::mutex mu;
    int n_cu = 0;
    // scratch slots reused across calls (host-pointer entry points)
    nmz::DevBuf buf[nmz::SLOT_COUNT];  // indexed by nmz::Slot
    nmz::DevBuf rank_keys;  // the signature's rank-key table (sig_rank_keys), built once per context; not scratch
    std::vector<nmz::DevBuf> pool;  // free plan buffers (DevBuf::pool), freed by nmz_close
    nmz::HostPin pin[2];             // pinned staging of plan inputs ([0] replayable plan, [1] its wavelet classes)
    bool wt_lds_attr = false;        // the wavelet-tree kernels' LDS attribute is set on this context's device
    // nmz_replayable_sweep_traces: a private second context (its stream takes the plan builds), an event per trace
    // in flight, and pinned staging for the top-k lists; created on first use
    nmz_ctx *helper = nullptr;
    hipEvent_t sweep_ev[3] = {nullptr, nullptr, nullptr};
    nmz::HostPin tkpin;
    NmzTiming timing;
    nmz_ctx() {
        for (int i = 0; i < nmz::SLOT_COUNT; ++i) buf[i].slot = nmz::SLOT_NAMES[i];
    }
};

namespace nmz {

// Records start/stop events around a kernel launch when timing is enabled.
struct KernelTimer {
    nmz_ctx *ctx;
    hipStream_t st;
    const char *name;
    hipEvent_t a = nullptr, b = nullptr;
    bool spans_only = false;
    KernelTimer(nmz_ctx *c, hipStream_t s, const char *n);
    ~KernelTimer();
    // a fresh span slot for a kernel that records its own execution span (nullptr when timing is off)
    unsigned long long *span();
};

// RAII: the caller's current HIP device is restored on return, so a call never changes the device of the thread
// that made it (torch or other HIP work on that thread keeps its own).
struct DeviceRestore {
    int prev = -1;
    DeviceRestore() {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    }
    ~DeviceRestore() {
        int cur = -1;
        if (prev >= 0 && hipGetDevice(&cur) == hipSuccess && cur != prev) (void)hipSetDevice(prev);
    }
};

// RAII: bind the calling OS thread to the context's device for the call (cgo threads migrate), then restore the
// caller's device.
struct CtxGuard {
    std::lock_guard<std::mutex> lk;
    DeviceRestore restore;
    int rc = NMZ_OK;
    explicit CtxGuard(nmz_ctx *c) : lk(c->mu) {
        if (hipSetDevice(c->device) != hipSuccess) rc = fail(NMZ_EHIP, "hipSetDevice failed");
    }
};

// Typed asynchronous copies: the byte count comes from the pointers' type, in size_t; a count of 0 copies nothing.
// A destination / source type mismatch does not compile.
template <typename T>
inline int copy_h2d(T *d_dst, const T *src, size_t count, hipStream_t st) {
    if (count) NMZ_HIP(hipMemcpyAsync(d_dst, src, count * sizeof(T), hipMemcpyHostToDevice, st));
    return NMZ_OK;
}
template <typename T>
inline int copy_d2h(T *dst, const T *d_src, size_t count, hipStream_t st) {
    if (count) NMZ_HIP(hipMemcpyAsync(dst, d_src, count * sizeof(T), hipMemcpyDeviceToHost, st));
    return NMZ_OK;
}
// the CSR of n traces: off[n + 1], then sym[off[n]]
inline int upload_csr(uint64_t *d_off, uint64_t *d_sym, const uint64_t *off, const uint64_t *sym, uint64_t n,
                      hipStream_t st) {
    NMZ_TRY(copy_h2d(d_off, off, n + 1, st));
    return copy_h2d(d_sym, sym, off[n], st);
}
// The seed strings of a host sweep. seed_csr_bytes: the bytes of seed_bytes (none in the decimal form, whose
// seeds are numbers); upload_seeds: seed_off[n_seeds + 1] and the bytes, nothing in the decimal form.
inline int seed_csr_bytes(const uint32_t *seed_off, const uint8_t *seed_bytes, uint64_t n_seeds, bool decimal,
                          uint64_t *sbytes) {
    *sbytes = (!decimal && n_seeds) ? seed_off[n_seeds] : 0;
    NMZ_CHECK(*sbytes == 0 || seed_bytes, "seed_bytes is NULL");
    return NMZ_OK;
}
inline int upload_seeds(uint32_t *d_soff, uint8_t *d_sb, const uint32_t *seed_off, const uint8_t *seed_bytes,
                        uint64_t n_seeds, bool decimal, hipStream_t st) {
    if (decimal || !n_seeds) return NMZ_OK;
    NMZ_TRY(copy_h2d(d_soff, seed_off, n_seeds + 1, st));
    return copy_h2d(d_sb, seed_bytes, seed_off[n_seeds], st);
}

// RAII: one synchronous host-form call on a context's stream. Declare it after the host-side variables that the
// call's device-to-host copies write and before anything else: every exit path then drains the stream before
// those variables (and the caller's arrays) go out of scope. After the drain it destroys the call's plan, if it
// owns one, and then hands `work`, the call's buffer from the context's pool (if the call took one), back to the
// pool. done() is the success path's one hipStreamSynchronize: it returns that status and disarms the drain.
struct HostCall {
    hipStream_t st;
    bool armed = true;
    void *plan = nullptr;
    void (*destroy)(void *) = nullptr;
    DevBuf work;
    explicit HostCall(nmz_ctx *c) : st(c->stream) { work.pool = &c->pool; }
    HostCall(const HostCall &) = delete;
    HostCall &operator=(const HostCall &) = delete;
    template <auto Destroy, typename P>
    void own_plan(P *p) {
        plan = p;
        destroy = [](void *q) { (void)Destroy(static_cast<P *>(q)); };
    }
    int done() {
        armed = false;
        NMZ_HIP(hipStreamSynchronize(st));
        return NMZ_OK;
    }
    ~HostCall() {
        if (armed) (void)hipStreamSynchronize(st);
        if (plan) destroy(plan);
        work.release();
    }
};

// ---------------------------------------------------------------------------
// FNV-1a 64 (Go hash/fnv New64a) and the low-byte decomposition used by the
// sweep kernels:  F_hint(h) = h * P^len + C_hint[h & 0xff]   (mod 2^64)
// The low byte of the FNV state evolves independently of the high bits
// (x * P mod 256 only sees x mod 256), so every XOR a hint byte applies is an
// additive offset that depends only on h & 0xff.
// ---------------------------------------------------------------------------
constexpr uint64_t FNV_OFFSET = 0xcbf29ce484222325ULL;
constexpr uint64_t FNV_PRIME = 0x100000001b3ULL;

__host__ __device__ inline uint64_t fnv_step(uint64_t h, uint32_t b) {
    return (h ^ (uint64_t)b) * FNV_PRIME;
}

__host__ __device__ inline uint64_t fnv_pow(uint32_t n) {
    uint64_t r = 1, b = FNV_PRIME;
    while (n) {
        if (n & 1) r *= b;
        b *= b;
        n >>= 1;
    }
    return r;
}

// ---------------------------------------------------------------------------
// u64 modulus by a launch constant m.
//   FAST   : 0 < m < 2^30, used through the carry decomposition (see replayable.hip)
//   GENERAL: any m > 0 (u64 remainder)
// ---------------------------------------------------------------------------
enum ModKind : int { MOD_ZERO = 0, MOD_FAST = 1, MOD_GENERAL = 2 };

struct ModParams {
    uint64_t m;
    uint32_t m32;
    uint32_t k64;   // 2^64 mod m (m < 2^32)
    uint32_t m_k64; // (m - k64) mod m, added when the 64-bit add carried (m < 2^32)
    uint64_t mu;    // floor(2^64 / m) for mod_barrett_small / mod_barrett64 (m < 2^32; 2^64 - 1 for m = 1)
    int kind;
    bool m32ok;     // 0 < m < 2^32: residues fit 32 bits (the order-query statistics apply)
};

inline ModParams make_mod(uint64_t m) {
    ModParams p{};
    p.m = m;
    p.m32ok = m != 0 && m < (1ULL << 32);
    if (p.m32ok) {
        p.m32 = (uint32_t)m;
        uint64_t k = (uint64_t)(((unsigned __int128)1 << 64) % m);
        p.k64 = (uint32_t)k;
        p.m_k64 = (uint32_t)((m - k) % m);
        p.mu = m == 1 ? ~0ULL : (uint64_t)(((unsigned __int128)1 << 64) / m);
    }
    p.kind = m == 0 ? MOD_ZERO : (m < (1ULL << 30) ? MOD_FAST : MOD_GENERAL);
    return p;
}

// v mod m for any 64-bit v and m < 2^31, mu = floor(2^64 / m) (2^64 - 1 for m = 1): q = floor(v * mu / 2^64)
// is floor(v / m) or one less, so r = v - q*m < 2m < 2^32 and only the low words are needed:
// r = v_lo - q_lo * m (mod 2^32), with v*mu = vl*mul + (vh*mul + vl*muh) 2^32 + vh*muh 2^64.
// high word of a 32 x 32-bit product (v_mul_hi_u32 on the device; the host decision path shares the code)
__host__ __device__ __forceinline__ uint32_t umulhi32(uint32_t a, uint32_t b) {
#ifdef __HIP_DEVICE_COMPILE__
    return __umulhi(a, b);
#else
    return (uint32_t)(((uint64_t)a * b) >> 32);
#endif
}
__host__ __device__ __forceinline__ uint64_t umulhi64(uint64_t a, uint64_t b) {
#ifdef __HIP_DEVICE_COMPILE__
    return __umul64hi(a, b);
#else
    return (uint64_t)(((unsigned __int128)a * b) >> 64);
#endif
}

__host__ __device__ __forceinline__ uint32_t mod_barrett_small(uint64_t v, uint32_t m, uint64_t mu) {
    const uint32_t vl = (uint32_t)v, vh = (uint32_t)(v >> 32);
    const uint32_t mul = (uint32_t)mu, muh = (uint32_t)(mu >> 32);
    const uint64_t a = (uint64_t)vh * mul + umulhi32(vl, mul);
    const uint64_t b = (uint64_t)vl * muh + (uint32_t)a;
    const uint32_t ql = vh * muh + (uint32_t)(a >> 32) + (uint32_t)(b >> 32);
    const uint32_t r = vl - ql * m;
    uint32_t t;
    return __builtin_sub_overflow(r, m, &t) ? r : t;
}

// v mod m for any 64-bit v and 0 < m < 2^32, mu = floor(2^64 / m): the quotient estimate is floor(v / m) or one
// less, so one conditional subtract.
__host__ __device__ __forceinline__ uint32_t mod_barrett64(uint64_t v, uint64_t m, uint64_t mu) {
    const uint64_t r = v - umulhi64(v, mu) * m;
    return (uint32_t)(r >= m ? r - m : r);
}

// Reduce s in [0, 3m) to [0, m) for m < 2^30 with two branch-free min steps.
__device__ inline uint32_t reduce3m(uint32_t s, uint32_t m) {
    s = min(s, s - m);
    return min(s, s - m);
}

// ---------------------------------------------------------------------------
// per-seed statistics accumulator
// ---------------------------------------------------------------------------
__host__ __device__ inline void stats_empty(nmz_sched_stats &s) {
    s.sum_delay_ns = 0;
    s.max_delay_ns = INT64_MIN;
    s.argmax_event = NMZ_NONE;
    s.n_fault = 0;
    s.first_fault = NMZ_NONE;
    s.flags = 0;
}

// ---------------------------------------------------------------------------
// launch helpers
// ---------------------------------------------------------------------------
inline unsigned ceil_div(uint64_t a, uint64_t b) { return (unsigned)((a + b - 1) / b); }

// seed bucketing by FNV low byte (shared by both sweeps): a counting sort with no global atomics. The prefix
// kernels hash blocks of BUCKET_BLK seeds and store each block's 256 bucket counts in its own row of b.hist (every
// row is written whole, so nothing needs zeroing); k_bucket_colscan turns each bucket's column of rows, in place,
// into the rows' offsets inside the bucket and the bucket's total; k_bucket_scatter scans the totals into the
// bucket starts and writes each block's seeds from start + row offset (block 0 also writes the starts and the work
// units). (Device-scope atomics on 256 shared counters from every block -- the previous form -- serialise on
// their words: ~11 ns each, 11 + 16 us per 2^20 seeds.)
constexpr uint32_t BUCKET_PT = 8;                 // seeds per thread of the prefix and scatter blocks (256 threads)
constexpr uint32_t BUCKET_BLK = 256 * BUCKET_PT;  // seeds per histogram row
constexpr size_t BUCKET_SMALL_U32 = 260 + 4 + 256;  // offset, n_units, total
inline uint64_t bucket_rows(uint64_t S) { return (S + BUCKET_BLK - 1) / BUCKET_BLK; }
inline size_t bucket_hist_u32(uint64_t S) { return (size_t)(bucket_rows(S) ? bucket_rows(S) : 1) * 256; }
struct Buckets {
    uint32_t *hist;        // [bucket_rows(S)][256]: the blocks' counts, then (k_bucket_colscan) their offsets
    uint32_t *offset;      // [257]
    uint32_t *n_units;     // [1]
    uint32_t *total;       // [256] bucket sizes
    uint4 *units;          // [max_units] {L, start, count, 0}
    uint64_t *sorted_h0;   // [S]
    uint32_t *sorted_idx;  // [S]
};

inline void buckets_small(uint32_t *small, Buckets &b) {
    b.offset = small;
    b.n_units = small + 260;
    b.total = small + 264;
}

// b.hist must already hold the bucket_rows(n_seeds) rows of counts (the caller's prefix kernel, blocks of
// BUCKET_BLK seeds); *zero_word, if given, is zeroed for the caller's work-item counter
int bucket_seeds_counted(hipStream_t st, const uint64_t *d_h0, uint64_t n_seeds, uint32_t seeds_per_unit,
                         Buckets &b, uint32_t *zero_word = nullptr);
// A/B and test knobs: an NMZ_* environment variable is read only when NMZ_AB=1 is set too, so that a production
// process's environment never changes which kernel runs or how a search deals its pairs over ranks
const char *ab_env(const char *name);


}  // namespace nmz
