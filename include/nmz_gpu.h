/*
 * nmz_gpu.h -- C ABI of libnmz_gpu.so, the MI355X (gfx950) engine behind
 * Namazu's explore-policy decision path and historystorage similarity search.
 *
 * This is the drop-in boundary: plain pointers and sizes, no HIP or torch
 * types, every call returns an int status (NMZ_OK == 0, <0 on error, message
 * in nmz_last_error()). A Go host binds it through cgo;
 * the Python host mirror in namazu_amd/ binds it through ctypes.
 *
 * Reference interfaces each entry point replaces (paths relative to the
 * reference tree, nmz/):
 *
 *   nmz_replayable_sweep*  -> Replayable.determineInterval / QueueEvent
 *                             explorepolicy/replayable/replayablepolicy.go:100-126
 *                             (FNV-1a64(seed || hint) % maxInterval), batched over
 *                             seeds x events.
 *   nmz_replayable_order_* -> the release times Replayable.QueueEvent gives,
 *                             replayablepolicy.go:100-126 (arrival + interval), checked
 *                             against event-order constraints per seed and batched over seeds.
 *   nmz_random_sweep*      -> Random.QueueEvent + makeActionForEvent
 *                             explorepolicy/random/randompolicy.go:300-316,332-346
 *                             + util/queue/impl.go:35-46,94-128 (Int63n delay,
 *                             Intn(999) fault draw), batched over seeds x events
 *                             under the deterministic per-event seeding contract
 *                             documented in DESIGN.md section 2.
 *   nmz_procset_*          -> Random's procPolicy.Action for ProcSetEvents
 *                             randompolicy.go:300-304, mild.go:44-57, extreme.go:44-63,
 *                             dirichlet.go:58-82 (one scheduling attribute per process),
 *                             on the host, on the device, and batched over seeds x events.
 *   nmz_random_params_resolve -> Random.LoadConfig's interval/probability
 *                             semantics randompolicy.go:156-228,332-340.
 *   nmz_ed_pairs / nmz_ed_allpairs_knn -> HistoryStorage similarity search
 *                             (optional interface next to Search /
 *                             SearchWithConverter, historystorage/historystorage.go:50-51,
 *                             naive/naive.go:235-257); distance 0 <=> SingleTrace.Equals
 *                             (util/trace/trace.go:29-31).
 *   nmz_ed_align_*         -> the same interface, extended: the edit script between
 *                             two traces (which events moved, are missing or were
 *                             replaced); an empty script <=> SingleTrace.Equals.
 *   nmz_script_moves_host / nmz_move_profile* / nmz_ed_diff_profile* -> the same
 *                             interface once more: the scripts of many pairs tallied per
 *                             event symbol (delivered later, earlier, dropped, extra).
 *
 * Buffers passed to the host-pointer entry points are borrowed for the call
 * only and never retained (cgo pointer rules). The *_dev entry points take
 * device pointers that are already resident in HBM plus a hipStream_t passed
 * as void*; they enqueue asynchronously on that stream.
 *
 * Threading: a context is bound to one device; calls on one context are
 * serialized by a mutex inside it and call hipSetDevice on entry, so a Go
 * caller may invoke them from any OS thread.
 */
#ifndef NMZ_GPU_H
#define NMZ_GPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NMZ_ABI_VERSION 1

/* status codes */
#define NMZ_OK 0
#define NMZ_EINVAL (-1)   /* bad argument (mirrors LoadConfig errors / queue panics) */
#define NMZ_EHIP (-2)     /* HIP runtime error */
#define NMZ_ENOMEM (-3)   /* device allocation failed */
#define NMZ_ERANGE (-4)   /* a decision needed more Go rng outputs than the kernel's closed form covers */
#define NMZ_EAGAIN (-5)   /* nothing became ready within the timeout (nmz_tbqueue_dequeue) */

/* per-event class bits for the random policy (one uint8 per event) */
#define NMZ_EV_PRIORITIZED 0x01u /* EntityID() in prioritizedEntities (randompolicy.go:335) */
#define NMZ_EV_FAULTABLE 0x02u   /* DefaultFaultAction() != nil: deferred Packet/Filesystem
                                    event (event_packet.go:45-47, event_filesystem.go:58-60) */

/* stats flags */
#define NMZ_STAT_RNG_OVERFLOW 0x01u

#define NMZ_NONE 0xffffffffu

/* Per-schedule statistics (one per seed), 32 bytes.
 * delays are time.Duration values (int64 ns). */
typedef struct nmz_sched_stats {
    uint64_t sum_delay_ns;  /* sum of delays, mod 2^64 (two's complement)          */
    int64_t max_delay_ns;   /* max delay (signed); INT64_MIN when there are no events */
    uint32_t argmax_event;  /* first event attaining max_delay_ns; NMZ_NONE if none */
    uint32_t n_fault;       /* number of fault actions chosen                        */
    uint32_t first_fault;   /* first event given a fault action; NMZ_NONE if none    */
    uint32_t flags;         /* NMZ_STAT_* bits                                       */
} nmz_sched_stats;

/* Failure-schedule candidate, ordered by (n_fault desc, sum_delay desc as int64,
 * seed asc). */
typedef struct nmz_topk_entry {
    uint64_t seed;
    int64_t sum_delay_ns;
    uint32_t n_fault;
    uint32_t first_fault;
} nmz_topk_entry;

/* Resolved random-policy parameters: the kernel consumes integers only.
 * Index 0 = ordinary entity, 1 = prioritized entity (x0.8 intervals). */
typedef struct nmz_random_params {
    int64_t min_ns[2];
    int64_t max_ns[2];
    int32_t fault_threshold; /* int(faultActionProbability * 1000.0) */
    uint32_t reserved;
} nmz_random_params;

typedef struct nmz_ctx nmz_ctx;

/* ---- context ---------------------------------------------------------- */
int nmz_open(int device, nmz_ctx **out);
int nmz_close(nmz_ctx *ctx);
const char *nmz_last_error(void); /* thread-local, valid until the next call on this thread */
int nmz_abi_version(void);
int nmz_device_count(int *count);
/* The context's own stream (hipStream_t as void*): what a NULL stream argument of the *_dev entry points means.
 * Each context's stream is created by the library (hipStreamCreateWithFlags), so contexts' streams are distinct
 * streams a caller may pipeline over (one plan per stream) and order its own work against. */
int nmz_ctx_stream(nmz_ctx *ctx, void **stream);

/* Kernel timing (HIP events recorded on the launch stream around the dominant
 * kernels: "replayable_sweep", "random_sweep", "procset_sweep", "order_sweep", "ed_tile"). on = 0 off, 1 events and
 * spans, NMZ_TIMING_SPANS (2) the kernels' own spans only (no event records between a
 * stream's launches: each record is a marker the queue waits on, ~6 us). */
#define NMZ_TIMING_SPANS 2
int nmz_timing_enable(nmz_ctx *ctx, int on);
int nmz_timing_read(nmz_ctx *ctx, const char *kernel, double *total_ms, uint64_t *count, int reset);
/* The same kernels' execution spans as the kernels record them (first workgroup start to last workgroup end,
 * wall_clock64()), so launches that wait on the stream for another stream's kernels are not charged the
 * wait ("replayable_sweep" on the order-query path): total_ms = the length of the union of the spans
 * (launches that overlap share their common time), count = launches. reset clears every kernel's spans. */
int nmz_timing_read_span(nmz_ctx *ctx, const char *kernel, double *total_ms, uint64_t *count, int reset);

/* FNV-1a 64 of each of n byte strings (CSR off[n+1] into bytes), one thread per string: the event
 * identities of a batch of events (their canonical JSON; Go hash/fnv New64a). */
int nmz_fnv1a64_batch(nmz_ctx *ctx, const uint64_t *off, const uint8_t *bytes, uint64_t n, uint64_t *out);

/* ---- online decisions on the calling host thread (no device work) ------------------------------------
 * The reference decides at enqueue, in the caller's goroutine (util/queue/impl.go:35-46,110-128;
 * replayablepolicy.go:116-126), and QueueEvent must not block (randompolicy_test.go:112-118): a GPU launch per
 * event (~100 us) is longer than the decision itself, so the online path decides on the host with the same
 * closed forms the kernels run (shared code: FNV, Go's seed reduction, the jump-ahead rngSource outputs,
 * Int63n / Intn rejection). Results equal nmz_*_decide and the sweeps bit for bit. Batch work (sweeps,
 * all-pairs search) stays on the GPU. */
int nmz_random_decide_host(uint64_t seed, const uint64_t *evhash, const uint8_t *evclass, uint32_t n_events,
                           const nmz_random_params *params, int64_t *delays, uint8_t *faults);
int nmz_replayable_decide_host(const uint8_t *seed, uint32_t seed_len, const uint32_t *hint_off,
                               const uint8_t *hint_bytes, uint32_t n_events, int64_t max_interval_ns,
                               int64_t *delays);
/* FNV-1a 64 of n byte strings (an event's canonical JSON -> its identity) */
int nmz_fnv1a64_batch_host(const uint64_t *off, const uint8_t *bytes, uint64_t n, uint64_t *out);

/* Time-bounded queue (util/queue/impl.go:64-128 BasicTBQueue; host only). One timer thread releases two kinds of
 * item, times in CLOCK_MONOTONIC ns (nmz_monotonic_ns):
 *   nmz_tbqueue_enqueue       a ranged item (min != max, impl.go:120-126): released at due_ns = enqueue + its drawn
 *                             duration;
 *   nmz_tbqueue_enqueue_fixed a fixed-duration item (min == max, impl.go:77-89,117-119): one FIFO lane whose head is
 *                             released at max(its enqueue, the previous fixed item's release) + duration, so a burst
 *                             of n items of duration d leaves at d, 2d, ..., nd, in enqueue order.
 * Equal due times release in enqueue order; consumers block in dequeue (the policy's ActionChan). A released item
 * records its due and release times, so release - due is the delivered-delay error of the online path. */
typedef struct nmz_tbqueue nmz_tbqueue;
int nmz_tbqueue_create(nmz_tbqueue **out);
/* close: no further enqueues; every consumer blocked in dequeue (and every later dequeue) returns NMZ_EAGAIN.
 * destroy: closes, joins the timer thread, waits until no call is inside dequeue, then frees the queue. A caller
 * must not start a call on the queue once destroy has begun (close first, let the consumers return, then
 * destroy: namazu_amd/explorepolicy.py ActionChannel.close). */
int nmz_tbqueue_close(nmz_tbqueue *q);
int nmz_tbqueue_destroy(nmz_tbqueue *q);
int64_t nmz_monotonic_ns(void);
int nmz_tbqueue_enqueue(nmz_tbqueue *q, uint64_t id, int64_t due_ns);
int nmz_tbqueue_enqueue_fixed(nmz_tbqueue *q, uint64_t id, int64_t enqueued_ns, int64_t duration_ns);
/* timeout_ns < 0: wait forever; NMZ_EAGAIN when nothing was released in time */
int nmz_tbqueue_dequeue(nmz_tbqueue *q, int64_t timeout_ns, uint64_t *id, int64_t *due_ns, int64_t *released_ns);
int nmz_tbqueue_stats(nmz_tbqueue *q, uint64_t *enqueued, uint64_t *released, uint64_t *dequeued);

/* ---- parameter resolution (host only, no device work) -------------------
 * min/max are time.Duration ns as parsed by LoadConfig; probability as float64.
 * Applies the prioritized x0.8 truncation in IEEE double exactly like
 * randompolicy.go:337-339, the threshold int(p*1000.0) of :310, and the
 * validity checks of :223-225 (probability) and util/queue/impl.go:36-38
 * (min > max). */
int nmz_random_params_resolve(int64_t min_ns, int64_t max_ns, double fault_probability,
                              nmz_random_params *out);

/* ---- replayable policy sweep ------------------------------------------
 * For each seed s (CSR: seed_off[n_seeds+1] into seed_bytes) and event e
 * (CSR: hint_off[n_events+1] into hint_bytes, the events' ReplayHint()):
 *     delay[s][e] = int64( FNV1a64(seed_s || hint_e) % uint64(max_interval_ns) )
 * and 0 for every event when max_interval_ns == 0 (replayablepolicy.go:101-104).
 * Outputs (each may be NULL):
 *   stats[n_seeds]
 *   delays[n_dump_seeds * n_events]  row-major, for the first n_dump_seeds seeds
 *   topk[k]   best k seeds by (sum_delay desc, seed index asc); entry .seed is
 *             the seed's index in the CSR.                                    */
int nmz_replayable_sweep(nmz_ctx *ctx, const uint32_t *seed_off, const uint8_t *seed_bytes,
                         uint64_t n_seeds, const uint32_t *hint_off, const uint8_t *hint_bytes,
                         uint32_t n_events, int64_t max_interval_ns, nmz_sched_stats *stats,
                         int64_t *delays, uint64_t n_dump_seeds, uint32_t k,
                         nmz_topk_entry *topk);

/* Device-resident variant (all pointers are device pointers; hipStream_t as void*).
 * The plan holds the per-event tables of one hint table and the scratch of one sweep
 * for up to max_seeds seeds. Sweeps through one plan must be ordered (one stream at a
 * time); concurrent sweeps on several streams take one plan each (bench.py pipelines
 * three). */
typedef struct nmz_replayable_plan nmz_replayable_plan;
int nmz_replayable_plan_create(nmz_ctx *ctx, const uint32_t *hint_off, const uint8_t *hint_bytes,
                               uint32_t n_events, int64_t max_interval_ns,
                               uint64_t max_seeds, nmz_replayable_plan **out);
/* The same, returning as soon as the build is enqueued on the context's stream (the host arrays may be
 * reused at once: they are staged in pinned memory). A sweep through the plan on any stream waits for the
 * build on the device; destroy waits for it and for the plan's sweeps. For a stream of traces: create trace
 * i + 1's plan (on a second context, so its build overlaps) while trace i sweeps. Plans the wavelet-tree plan
 * kernel does not build in one launch (a class of 4,096 events or more, order-query or per-decision plans)
 * are built synchronously as by nmz_replayable_plan_create. */
int nmz_replayable_plan_create_async(nmz_ctx *ctx, const uint32_t *hint_off, const uint8_t *hint_bytes,
                                     uint32_t n_events, int64_t max_interval_ns, uint64_t max_seeds,
                                     nmz_replayable_plan **out);
/* A prepared seed set for sweeping one set of seeds over many traces' plans: the seeds' prefix hashes (FNV of the
 * seed bytes), bucketed by table row once, instead of per sweep. d_seed_off / d_seed_bytes: device CSR of the seed
 * strings, or d_seed_off == NULL: the decimal strings of dec_lo .. dec_lo + n_seeds - 1. Synchronous; the set may be
 * swept through any plan on the same device and stream (results identical to nmz_replayable_sweep_topk_dev and
 * nmz_replayable_sweep_decimal_topk_dev over the same seeds). Destroy waits for the device. */
typedef struct nmz_replayable_seeds nmz_replayable_seeds;
int nmz_replayable_seeds_create(nmz_ctx *ctx, const uint32_t *d_seed_off, const uint8_t *d_seed_bytes,
                                uint64_t n_seeds, uint64_t dec_lo, nmz_replayable_seeds **out);
int nmz_replayable_seeds_destroy(nmz_replayable_seeds *seeds);
/* nmz_replayable_sweep_topk_dev over a prepared seed set: stats for every seed of the set, and (k > 0) the top-k
 * with seed = seed0 + the seed's index. */
int nmz_replayable_sweep_seeds_topk_dev(nmz_replayable_plan *plan, const nmz_replayable_seeds *seeds, uint64_t seed0,
                                        uint32_t k, nmz_sched_stats *d_stats, nmz_topk_entry *d_topk, void *stream);
/* A batch of recorded traces over one decimal seed range (the reference seeds "lo" .. "lo + n - 1",
 * replayablepolicy.go:74-87): for every trace t (hint CSR hint_off[t] / hint_bytes[t], n_events[t] hints) its own
 * plan, the sweep of all n_seeds seeds and the top-k failure candidates into topk[t * k .. t * k + k) (as
 * nmz_replayable_sweep_decimal_topk_dev). Pipelined inside: the seeds are prepared once, trace t + 2's plan builds
 * while trace t sweeps (on a private second context the call opens on first use), top-k lists come back while
 * the next trace sweeps. Host arrays only; synchronous. 1 <= k <= 256. */
int nmz_replayable_sweep_traces(nmz_ctx *ctx, uint32_t n_traces, const uint32_t *const *hint_off,
                                const uint8_t *const *hint_bytes, const uint32_t *n_events, int64_t max_interval_ns,
                                uint64_t seed_lo, uint64_t n_seeds, uint32_t k, nmz_topk_entry *topk);
/* Waits for the plan's build and for the sweeps enqueued through it (not for the device or other streams). */
int nmz_replayable_plan_destroy(nmz_replayable_plan *plan);
/* Which statistics kernel the plan's sweeps take (diagnostic): 2 = wavelet-tree statistics (k_replayable_sweep_wt,
 * the default when 0 < max_interval < 2^32, the trace has <= 65,536 events -- a hint-length class of 4,096 or more
 * splits into sub-segments -- and the row image fits LDS),
 * 1 = order-query statistics (k_replayable_sweep_oq), 0 = per-decision sweeps; -1 for a NULL plan. The environment
 * variable NMZ_REPLAY_WT=0 at plan creation skips the wavelet trees (A/B runs). */
int nmz_replayable_plan_kernel(const nmz_replayable_plan *plan);
/* The form of a wavelet-tree plan (diagnostic; an error for a plan whose sweeps take another kernel): *bb = log2 of
 * the rank blocks' width (5, 6 or 7), *planes = 1 when the segments hold rank-block planes in place of the levels
 * above the blocks (64-rank blocks and a row image of at most 128 KB; NMZ_WT_PLANES=0 at plan creation keeps the
 * levels, A/B runs), *image_bytes = the bytes of one row image (staged into LDS per sweep workgroup). Any of the three
 * may be NULL. */
int nmz_replayable_plan_wt_info(const nmz_replayable_plan *plan, uint32_t *bb, uint32_t *planes,
                                uint64_t *image_bytes);
int nmz_replayable_sweep_dev(nmz_replayable_plan *plan, const uint32_t *d_seed_off,
                             const uint8_t *d_seed_bytes, uint64_t n_seeds,
                             nmz_sched_stats *d_stats, void *stream);
/* The same plus the top-k failure candidates (d_topk[k], k <= 256, by sum_delay desc then seed asc,
 * .seed = seed0 + seed index), enqueued in one call. Results equal nmz_replayable_sweep_dev +
 * nmz_topk_select_dev(seed0, k).
 * Same reference path as nmz_replayable_sweep (replayablepolicy.go:100-114); top-k is SURVEY A7. */
int nmz_replayable_sweep_topk_dev(nmz_replayable_plan *plan, const uint32_t *d_seed_off,
                                  const uint8_t *d_seed_bytes, uint64_t n_seeds, uint64_t seed0,
                                  uint32_t k, nmz_sched_stats *d_stats, nmz_topk_entry *d_topk,
                                  void *stream);

/* The same sweep for the seeds "seed_lo", "seed_lo+1", ... "seed_lo+n_seeds-1": the decimal strings of those
 * uint64 integers (strconv.FormatUint, wrapping past 2^64), generated on the device, so a sweep over a range of
 * integer seeds needs no seed CSR in memory. Top-k .seed = the seed's integer value (seed_lo + index). Results
 * equal nmz_replayable_sweep_topk_dev over the CSR of those strings with seed0 = seed_lo. n_seeds <= max_seeds
 * of the plan. Same reference path (replayablepolicy.go:74-87 seed string, :100-114 interval). */
int nmz_replayable_sweep_decimal_topk_dev(nmz_replayable_plan *plan, uint64_t seed_lo, uint64_t n_seeds, uint32_t k,
                                          nmz_sched_stats *d_stats, nmz_topk_entry *d_topk, void *stream);

/* Online decisions (Replayable.QueueEvent -> determineInterval, replayablepolicy.go:100-126):
 * delays[e] = the interval of seed (seed_len bytes) for each of n_events pending events' hints
 * (CSR hint_off[n_events+1] into hint_bytes). No plan or tables: a batch of the events queued
 * since the last call, one thread per event. Synchronous; scratch is owned by the context. */
int nmz_replayable_decide(nmz_ctx *ctx, const uint8_t *seed, uint32_t seed_len, const uint32_t *hint_off,
                          const uint8_t *hint_bytes, uint32_t n_events, int64_t max_interval_ns, int64_t *delays);

/* ---- replayable policy: seeds against event-order constraints ----------------
 * Replayable.QueueEvent releases every event at arrival + determineInterval(event)
 * (replayablepolicy.go:100-126), so a seed is a delivery order. For one trace the caller gives the hints
 * (CSR, n_events, as above), arrival_ns[n_events] (int64, when each event reached QueueEvent, any origin) and
 * n_constraints constraints {before, after, margin_ns}. For seed s:
 *     release[s][e] = arrival_ns[e] + delay[s][e]      (delay as nmz_replayable_sweep; 0 when max_interval_ns == 0)
 *     slack[s][c]   = release[s][after_c] - release[s][before_c] - margin_c
 * Constraint c is satisfied iff slack >= 0: event `before` is delivered at least margin_ns ahead of `after`
 * (margin_ns >= 1 makes the order strict; use a margin of timer-jitter size, the reference sleeps in real time).
 * Limits, each NMZ_EINVAL with a message: 1 <= n_constraints <= 64; before != after, both < n_events;
 * 0 <= arrival_ns <= 2^61; 1 <= margin_ns <= 2^61; 0 <= max_interval_ns <= 2^61 (every slack then fits int64 and
 * INT64_MIN stays free as the top-k sentinel). Two events with equal hints are legal: their slack is the same for
 * every seed.
 * Seeds are ranked by (n_satisfied desc, min_slack_ns desc, seed asc): among seeds satisfying everything, the one
 * whose tightest constraint has the most room. That is nmz_topk_entry's order, and the sweeps write their top-k as
 * nmz_topk_entry with
 *     n_fault = n_satisfied, sum_delay_ns = min_slack_ns, first_fault = argmin_constraint,
 *     seed = the CSR index (+ seed0) or the decimal value, as the sweeps above,
 * and the same sentinel {UINT64_MAX, INT64_MIN, 0, NMZ_NONE} past n_seeds, so nmz_topk_merge_dev merges the lists of
 * several sweeps and namazu_amd/replay.py turns them into NMZ_REPLAY_SEED unchanged. */
typedef struct nmz_order_constraint {
    uint32_t before;   /* event that must be released first      */
    uint32_t after;    /* event that must be released later      */
    int64_t margin_ns; /* by at least this much                  */
} nmz_order_constraint;

/* Per-seed statistics of an order sweep, 24 bytes. */
typedef struct nmz_order_stats {
    uint64_t sat_mask;          /* bit c set <=> constraint c is satisfied          */
    int64_t min_slack_ns;       /* minimum slack over the constraints               */
    uint32_t n_satisfied;       /* popcount(sat_mask)                               */
    uint32_t argmin_constraint; /* the first constraint attaining min_slack_ns      */
} nmz_order_stats;

/* One seed on the calling host thread, no device work (replayablepolicy.go:100-126): the statistics (may be NULL)
 * and, if slack != NULL, slack[n_constraints]. Vets a candidate seed before a replay. */
int nmz_replayable_order_host(const uint8_t *seed, uint32_t seed_len, const uint32_t *hint_off,
                              const uint8_t *hint_bytes, uint32_t n_events, int64_t max_interval_ns,
                              const int64_t *arrival_ns, const nmz_order_constraint *constraints,
                              uint32_t n_constraints, nmz_order_stats *stats, int64_t *slack);
/* The plan holds the per-constraint device tables of one trace and the scratch of one sweep of up to max_seeds
 * (< 2^32) seeds; host arrays are borrowed for the call. Like the other plans it serves one stream at a time (two
 * streams take one plan each). Destroy waits for the plan's sweeps. Same reference lines
 * (replayablepolicy.go:100-126). */
typedef struct nmz_replayable_order_plan nmz_replayable_order_plan;
int nmz_replayable_order_plan_create(nmz_ctx *ctx, const uint32_t *hint_off, const uint8_t *hint_bytes,
                                     uint32_t n_events, int64_t max_interval_ns, const int64_t *arrival_ns,
                                     const nmz_order_constraint *constraints, uint32_t n_constraints,
                                     uint64_t max_seeds, nmz_replayable_order_plan **out);
int nmz_replayable_order_plan_destroy(nmz_replayable_order_plan *plan);
/* The seeds "seed_lo" .. "seed_lo + n_seeds - 1" (decimal strings generated on the device, wrapping past 2^64 as
 * nmz_replayable_sweep_decimal_topk_dev; replayablepolicy.go:74-87 seed string, :100-126 release times), enqueued on
 * `stream` (NULL = the context's). d_stats[n_seeds] may be NULL: the sweep then writes only d_topk[k] (k <= 256;
 * k == 0: no top-k), the hot form. Top-k .seed = the seed's integer value. */
int nmz_replayable_order_sweep_decimal_dev(nmz_replayable_order_plan *plan, uint64_t seed_lo, uint64_t n_seeds,
                                           uint32_t k, nmz_order_stats *d_stats /* may be NULL */,
                                           nmz_topk_entry *d_topk, void *stream);
/* The same for arbitrary seed strings (device CSR d_seed_off[n_seeds + 1] into d_seed_bytes; the empty seed is the
 * reference's default, replayablepolicy.go:74-81). Top-k .seed = seed0 + the seed's index. */
int nmz_replayable_order_sweep_dev(nmz_replayable_order_plan *plan, const uint32_t *d_seed_off,
                                   const uint8_t *d_seed_bytes, uint64_t n_seeds, uint64_t seed0, uint32_t k,
                                   nmz_order_stats *d_stats /* may be NULL */, nmz_topk_entry *d_topk, void *stream);
/* Host pointers, synchronous, built on the plan (replayablepolicy.go:100-126): stats[n_seeds] and topk[k] may each
 * be NULL; k <= 256. Top-k .seed = the seed's index in the CSR, or its integer value for the decimal form. */
int nmz_replayable_order_sweep(nmz_ctx *ctx, const uint32_t *seed_off, const uint8_t *seed_bytes, uint64_t n_seeds,
                               const uint32_t *hint_off, const uint8_t *hint_bytes, uint32_t n_events,
                               int64_t max_interval_ns, const int64_t *arrival_ns,
                               const nmz_order_constraint *constraints, uint32_t n_constraints, uint32_t k,
                               nmz_order_stats *stats, nmz_topk_entry *topk);
int nmz_replayable_order_sweep_decimal(nmz_ctx *ctx, uint64_t seed_lo, uint64_t n_seeds, const uint32_t *hint_off,
                                       const uint8_t *hint_bytes, uint32_t n_events, int64_t max_interval_ns,
                                       const int64_t *arrival_ns, const nmz_order_constraint *constraints,
                                       uint32_t n_constraints, uint32_t k, nmz_order_stats *stats,
                                       nmz_topk_entry *topk);

/* ---- random policy sweep ------------------------------------------------
 * Seeds are the integers seed0 .. seed0+n_seeds-1. For seed s and event e
 * (evhash[e], evclass[e] = NMZ_EV_* bits) the decision is made by a fresh
 *     rng = rand.New(rand.NewSource(int64(FNV1a64(le64(s) || le64(evhash[e])))))
 * drawing, in this order,
 *     delay = rng.Int63n(max-min) + min   if min != max  (else delay = min, no draw)
 *     fault = rng.Intn(999) < fault_threshold            if NMZ_EV_FAULTABLE
 * with (min,max) = params->{min,max}_ns[prioritized].
 * Outputs (each may be NULL): stats[n_seeds]; delays/faults[n_dump_seeds*n_events];
 * topk[k] by (n_fault desc, sum_delay desc, seed asc), .seed = the seed value. */
int nmz_random_sweep(nmz_ctx *ctx, uint64_t seed0, uint64_t n_seeds, const uint64_t *evhash,
                     const uint8_t *evclass, uint32_t n_events, const nmz_random_params *params,
                     nmz_sched_stats *stats, int64_t *delays, uint8_t *faults,
                     uint64_t n_dump_seeds, uint32_t k, nmz_topk_entry *topk);

/* Online decisions (Random.QueueEvent -> makeActionForEvent, randompolicy.go:300-346): the delay and
 * fault choice of one seed for each of n_events pending events, the same decision as
 * nmz_random_sweep makes for that seed and event. No plan; synchronous. */
int nmz_random_decide(nmz_ctx *ctx, uint64_t seed, const uint64_t *evhash, const uint8_t *evclass,
                      uint32_t n_events, const nmz_random_params *params, int64_t *delays, uint8_t *faults);

/* Device-resident variant: per-event tables are built once in the plan; the
 * sweep enqueues on `stream` and writes d_stats[n_seeds] (device memory). As for
 * replayable plans, one plan serves one stream at a time. */
typedef struct nmz_random_plan nmz_random_plan;
int nmz_random_plan_create(nmz_ctx *ctx, const uint64_t *evhash, const uint8_t *evclass,
                           uint32_t n_events, const nmz_random_params *params, uint64_t max_seeds,
                           nmz_random_plan **out);
int nmz_random_plan_destroy(nmz_random_plan *plan);
int nmz_random_sweep_dev(nmz_random_plan *plan, uint64_t seed0, uint64_t n_seeds,
                         nmz_sched_stats *d_stats, void *stream);

/* ---- random policy: ProcSetEvent decisions (procPolicy) -----------------------
 * makeActionForEvent hands every ProcSetEvent to the policy's procPolicy
 * (randompolicy.go:300-304), which answers with a ProcSetSchedAction: one
 * scheduling attribute per process of the set. The decision for (seed s, event e)
 * uses the generator of nmz_random_sweep and draws, in order,
 *   1. the delay, exactly as nmz_random_sweep (QueueEvent treats the event like any
 *      other; a ProcSetEvent is not deferred, so there is no fault draw);
 *   2. with n = n_procs[e], the sub-policy's draws:
 *      mild      (mild.go:44-57)     slot i: nice = -20 + Int31n(40); policy SCHED_BATCH
 *                                    if use_batch, else SCHED_NORMAL;
 *      extreme   (extreme.go:44-63)  `prioritized` times: mark slot Int31n(n) (a set);
 *                                    then, in slot order, a marked slot is
 *                                    {SCHED_RR, priority = Int31n(10)}, the others
 *                                    {SCHED_BATCH}; prioritized <= 0: no draws;
 *      dirichlet (dirichlet.go:58-82) slot i: reset = Intn(999) < reset_threshold;
 *                                    a reset slot is {SCHED_NORMAL}, the others
 *                                    {SCHED_DEADLINE, SCHED_FLAG_RESET_ON_FORK}. The
 *                                    runtime ratios come from a second, clock-seeded
 *                                    generator (dirichlet.go:29-31) and are not part
 *                                    of this interface.
 * Limits (the closed forms cover 607 generator outputs): n_procs[e] <= 512 and
 * prioritized <= 256, NMZ_EINVAL beyond; extreme with n = 0 and prioritized > 0
 * (Go's Int31n(0) panics) and dirichlet with n = 0 ("has no process", dirichlet.go:43-45)
 * are NMZ_EINVAL. evclass may carry NMZ_EV_PRIORITIZED only. */
#define NMZ_PROC_MILD 0
#define NMZ_PROC_EXTREME 1
#define NMZ_PROC_DIRICHLET 2
#define NMZ_PROCSET_MAX_PROCS 512
#define NMZ_PROCSET_MAX_PRIORITIZED 256

typedef struct nmz_procset_params {
    int32_t policy;          /* NMZ_PROC_*                                              */
    int32_t use_batch;       /* PPPMild.UseBatch                                        */
    int32_t prioritized;     /* PPPExtreme.Prioritized                                  */
    int32_t reset_threshold; /* int(PPPDirichlet.ResetProbability * 1000.0)             */
} nmz_procset_params;

/* loadProcConfig's checks (randompolicy.go:230-270): proc_policy "" or NULL means mild; errors
 * "bad procPolicy %s" and "bad procPolicyParam.resetProbability %f" (:262-267); prioritized above
 * NMZ_PROCSET_MAX_PRIORITIZED is NMZ_EINVAL. Host only. */
int nmz_procset_params_resolve(const char *proc_policy, int use_batch, int prioritized, double reset_probability,
                               nmz_procset_params *out);

/* One process's attribute, 16 bytes; policy and flags are the Linux numbers (linuxsched.SchedAttr):
 * SCHED_NORMAL 0, SCHED_RR 2, SCHED_BATCH 3, SCHED_DEADLINE 6; SCHED_FLAG_RESET_ON_FORK 1. */
typedef struct nmz_proc_attr {
    uint32_t policy;
    int32_t nice;
    uint32_t priority;
    uint32_t flags;
} nmz_proc_attr;

/* Per-seed statistics of a ProcSet sweep, 32 bytes. The favour score of one process in one decision (higher =
 * more CPU): mild -nice (-19..20); extreme 1 + priority if SCHED_RR, else 0; dirichlet 1 if reset, else 0. */
typedef struct nmz_procset_stats {
    uint64_t sum_delay_ns; /* sum of delays, mod 2^64                                          */
    int64_t score_sum;     /* favour score over every process of every event                    */
    int64_t target_score;  /* favour score over target_slot[e] of every event                   */
    uint32_t n_special;    /* mild: processes with nice < 0; extreme: SCHED_RR; dirichlet: resets */
    uint32_t flags;        /* NMZ_STAT_* bits                                                   */
} nmz_procset_stats;

typedef struct nmz_procset_topk_entry {
    uint64_t seed;
    int64_t target_score;
} nmz_procset_topk_entry;

/* procPolicy.Action (mild.go:30-40, extreme.go:30-40, dirichlet.go:38-51) for one seed on the calling thread, no
 * device work: delays[n_events] and attrs[sum of n_procs], event e's processes at the prefix sum of n_procs[0..e).
 * Shares its decision code with the kernels, as nmz_random_decide_host does. */
int nmz_procset_decide_host(uint64_t seed, const uint64_t *evhash, const uint8_t *evclass, const uint32_t *n_procs,
                            uint32_t n_events, const nmz_random_params *random_params,
                            const nmz_procset_params *procset_params, int64_t *delays, nmz_proc_attr *attrs);
/* The same decisions (same reference lines) on the device, one thread per event. Synchronous. */
int nmz_procset_decide(nmz_ctx *ctx, uint64_t seed, const uint64_t *evhash, const uint8_t *evclass,
                       const uint32_t *n_procs, uint32_t n_events, const nmz_random_params *random_params,
                       const nmz_procset_params *procset_params, int64_t *delays, nmz_proc_attr *attrs);
/* procPolicy.Action (the same reference lines) batched over seeds seed0 .. seed0 + n_seeds - 1 (wrapping past 2^64 as
 * nmz_random_sweep) x events. target_slot[e] is a slot < n_procs[e] or NMZ_NONE; NULL = all NMZ_NONE.
 * Outputs (each may be NULL): stats[n_seeds]; delays[n_dump_seeds * n_events] and attrs[n_dump_seeds * sum of
 * n_procs] (row-major, one row per seed, laid out as nmz_procset_decide_host's) for the first n_dump_seeds seeds;
 * topk[k], k <= 256, by target_score (descending if `descending`, else ascending), then seed ascending, .seed = the
 * seed value; entries past n_seeds are {UINT64_MAX, INT64_MIN}. */
int nmz_procset_sweep(nmz_ctx *ctx, uint64_t seed0, uint64_t n_seeds, const uint64_t *evhash, const uint8_t *evclass,
                      const uint32_t *n_procs, const uint32_t *target_slot, uint32_t n_events,
                      const nmz_random_params *random_params, const nmz_procset_params *procset_params,
                      nmz_procset_stats *stats, int64_t *delays, nmz_proc_attr *attrs, uint64_t n_dump_seeds,
                      uint32_t k, int descending, nmz_procset_topk_entry *topk);

/* Top-k selection over device-resident stats (seed value = seed0 + index).
 * k <= 256 (here and for the sweeps' topk outputs); NMZ_EINVAL otherwise. */
int nmz_topk_select_dev(nmz_ctx *ctx, const nmz_sched_stats *d_stats, uint64_t n, uint64_t seed0,
                        uint32_t k, nmz_topk_entry *d_out, void *stream);
/* Merge n_lists top-k lists (d_lists[n_lists][k], each sorted as the sweeps write them: n_fault desc, sum_delay
 * desc, seed asc) into the best k (d_out[k]): the lists of several sweeps over disjoint seed ranges (successive
 * batches of one job, or the shards of one rank) become the job's top-k. d_lists and d_scratch (same size) are
 * overwritten. k <= 256. */
int nmz_topk_merge_dev(nmz_ctx *ctx, nmz_topk_entry *d_lists, uint64_t n_lists, uint32_t k,
                       nmz_topk_entry *d_scratch, nmz_topk_entry *d_out, void *stream);

/* ---- trace similarity (banded Levenshtein over event-hash sequences) ------
 * Traces in CSR: off[n_traces+1] (element offsets) into sym[] (uint64 event
 * hashes). ED_w(a,b) = min(D(n,m), w+1) where D is unit-cost Levenshtein
 * restricted to cells |i-j| <= w (cells outside the band are +inf).
 * ED_w == 0  <=>  the traces are equal element-wise (SingleTrace.Equals). */
int nmz_ed_pairs(nmz_ctx *ctx, const uint64_t *off, const uint64_t *sym, uint32_t n_traces,
                 const uint32_t *pairs /* [2*n_pairs] */, uint64_t n_pairs, uint32_t band,
                 uint32_t *dist /* [n_pairs] */);

/* All pairs i != j; for each trace the k nearest others by (dist asc, id asc).
 * knn_id/knn_dist are [n_traces * k]; missing entries are NMZ_NONE. */
int nmz_ed_allpairs_knn(nmz_ctx *ctx, const uint64_t *off, const uint64_t *sym,
                        uint32_t n_traces, uint32_t band, uint32_t k, uint32_t *knn_id,
                        uint32_t *knn_dist);

/* Device-resident variant: the plan remaps symbols to dense ids and builds the
 * lane-interleaved candidate layout once; searches then run on resident data.
 * d_knn_keys[n_traces * k] (device) receives sorted keys (dist << 32 | id),
 * UINT64_MAX for missing entries. k in [1, 64]. */
typedef struct nmz_ed_plan nmz_ed_plan;
int nmz_ed_plan_create(nmz_ctx *ctx, const uint64_t *off, const uint64_t *sym, uint32_t n_traces,
                       uint32_t band, nmz_ed_plan **out);
/* The same plan from event hashes already in device memory: off (host, n_traces + 1 offsets) and d_sym (device,
 * off[n_traces] u64, read during the call). Multi-GPU callers upload 1/N of the symbols per device and all_gather
 * them over RCCL instead of pushing the whole store through every device's PCIe link. */
int nmz_ed_plan_create_dev(nmz_ctx *ctx, const uint64_t *off, const uint64_t *d_sym, uint32_t n_traces,
                           uint32_t band, nmz_ed_plan **out);
/* Plan options (bit flags) of nmz_ed_plan_create_opts. 0 is the product's choice; the others select the
 * alternative forms of the bit-parallel search, for A/B runs and tests. Whichever form a plan takes, a shard owns
 * the same pairs (whole 64-query blocks, nmz_ed_block_shard), so within ONE process the shards of a search may run on
 * plans of different forms and still partition the pairs (tests/test_ed_gpu.py checks this). The multi-rank paths do
 * not allow the mix: the device groups and namazu_amd/dist.check_ed_plans require equal fingerprints, which include
 * the form bits, and fail with NMZ_EINVAL otherwise. The NMZ_ED_* environment knobs that add to these are read only
 * when NMZ_AB=1 is set. */
#define NMZ_ED_OPT_SINGLE_KERNEL 1u /* no two-phase search: the single kernel with its in-workgroup pre-filter */
#define NMZ_ED_OPT_NO_QGRAM 2u      /* no q-gram lower-bound filter (the single kernel, without the filter) */
#define NMZ_ED_OPT_COMPACT 4u       /* compact per-workgroup Peq tables even when the direct tables fit */
#define NMZ_ED_OPT_HOST_BUILD 8u    /* the plan's streams built on the host instead of the device */
/* sym (host) or d_sym (device, read during the call): exactly one of them when the store is not empty */
int nmz_ed_plan_create_opts(nmz_ctx *ctx, const uint64_t *off, const uint64_t *sym, const uint64_t *d_sym,
                            uint32_t n_traces, uint32_t band, uint32_t opts, nmz_ed_plan **out);
/* The plan's fingerprint, 8 words: version, kernel kind | band << 8 | template band << 40, n_traces, total
 * symbols, two-phase | q-gram << 1 | compact << 2, block-row queries | pool << 32, FNV-1a 64 of the offsets, alphabet
 * size. Ranks that search one store together must hold equal fingerprints: the device groups all_gather them when
 * a plan is created and fail with NMZ_EINVAL when they differ. */
#define NMZ_ED_FP_WORDS 8
#define NMZ_ED_FP_VERSION 1u
int nmz_ed_plan_fingerprint(const nmz_ed_plan *plan, uint64_t *fp /* [NMZ_ED_FP_WORDS] */);
int nmz_ed_plan_destroy(nmz_ed_plan *plan);
int nmz_ed_plan_is_fast(const nmz_ed_plan *plan);
int nmz_ed_allpairs_knn_dev(nmz_ed_plan *plan, uint32_t k, uint64_t *d_knn_keys, void *stream);
/* Multi-GPU: shard `shard` of `n_shards` processes every n_shards-th work chunk;
 * its keys are partial lists. nmz_knn_merge_dev merges n_parts partial lists
 * ([n_parts][n_traces][k], e.g. after an RCCL all_gather), and nmz_ed_knn_fill_dev
 * then completes the merged lists: on a bit-parallel plan (nmz_ed_plan_is_fast == 2) a
 * shard lists only its pairs within the band, and every other pair's result is band + 1,
 * so the merged lists take (band + 1, id) for the smallest ids not listed (not the trace
 * itself), in increasing id, up to k. On other plans the fill leaves complete lists
 * unchanged. (nmz_ed_allpairs_knn[_dev] fill by themselves.) */
/* Host-only (no device work): the shard that owns query block qb (queries 64 qb .. 64 qb + 63) of the
 * bit-parallel search (both forms: two-phase and the single kernel) under nmz_ed_allpairs_knn_shard_dev with n_shards shards: every pair (i, j), i < j, belongs
 * to the shard of block i / 64, in rotated snake order (in each period of 2 n_shards blocks, block r and its mirror
 * 2 n_shards - 1 - r form pair p = min(r, 2 n_shards - 1 - r), which goes to shard (p + period) mod n_shards). A
 * fixed rule, the same in every process (no environment knob). A shard whose entry lists exceed the two-phase limit
 * runs its own query blocks in batches, so every shard of a search deals by this rule. tests/test_dist_cpu.py deals
 * pairs by it. */
uint32_t nmz_ed_block_shard(uint32_t qb, uint32_t n_shards);
int nmz_ed_allpairs_knn_shard_dev(nmz_ed_plan *plan, uint32_t k, uint32_t shard, uint32_t n_shards,
                                  uint64_t *d_knn_keys, void *stream);
int nmz_knn_merge_dev(nmz_ctx *ctx, const uint64_t *d_parts, uint32_t n_parts, uint32_t n_traces,
                      uint32_t k, uint64_t *d_out, void *stream);
int nmz_ed_knn_fill_dev(nmz_ed_plan *plan, uint32_t k, uint64_t *d_knn_keys, void *stream);
/* Single queries against a resident store (HistoryStorage similarity search; the reference's own
 * search re-decodes every stored trace per query, naive.go:235-252 "FIXME: quite ineffective"):
 * the plan's stored traces stay on the device; each of n_queries query traces (CSR q_off/q_sym,
 * u64 event hashes, any length) gets its k nearest stored traces by (ED_band asc, id asc), ED_band
 * as in nmz_ed_pairs. knn_id/knn_dist are [n_queries * k], NMZ_NONE where fewer than k traces
 * exist. Any plan and band: bit-parallel plans (band <= 64) run k_ed_bv's query form, wide plans
 * (64 < band <= 8,192) k_ed_wide_query, the others (and queries longer than the plan's kernel
 * takes) a generic per-pair kernel over the resident store. 1 <= k <= 64. Synchronous. */
int nmz_ed_plan_query_knn(nmz_ed_plan *plan, const uint64_t *q_off, const uint64_t *q_sym, uint32_t n_queries,
                          uint32_t k, uint32_t *knn_id, uint32_t *knn_dist);
/* Work counters of the plan's latest search (synchronises `stream`, NULL = the context's stream).
 * out[NMZ_ED_NCOUNTERS]: the bit-parallel band kernel (nmz_ed_plan_is_fast == 2) fills
 *   [0] pairs that ran the DP, [1] pairs whose result is <= band (in band),
 *   [2] candidate x 32-column blocks executed (each block steps 2 query columns per candidate),
 *   [3] candidates that ran the DP, [4] live query-blocks (blocks x queries still running),
 *   [5] pairs inside the length band whose result the q-gram lower bound settled at band + 1
 *       without a DP;
 * other kernels keep no counters and leave zeros. Diagnostics for the bench, not part of the
 * reference interface. */
#define NMZ_ED_NCOUNTERS 6
int nmz_ed_plan_counters(nmz_ed_plan *plan, uint64_t *out, void *stream);
/* Test hook, not part of the reference interface: the two-phase search's offset kernels (k_tp_reduce, k_tp_scan)
 * on caller data. d_cnt[n] (device) -> d_poff[n + 1] = exclusive prefix sums of the counts mod 2^32,
 * d_ioff[n + 1] = exclusive prefix sums of ceil(count / item) mod 2^32, *d_tot = the 64-bit count total;
 * item a power of two. Enqueued on `stream` (NULL = the context's stream), synchronised before it returns. */
int nmz_debug_tp_offsets(nmz_ctx *ctx, const uint32_t *d_cnt, uint32_t n, uint32_t item, uint32_t *d_poff,
                         uint32_t *d_ioff, uint64_t *d_tot, void *stream);

/* ---- trace equality classes (nmz tools visualize) ------------------------
 * Replaces the O(n^2) loops of cli/tools/visualize.go:51-172 (gnuplot): trace i is a
 * repeat iff an earlier trace equals it.
 *   entity == NULL: exact mode (seenBefore, :51-60) -- sequence equality of sym[], i.e.
 *       SingleTrace.Equals / AreActionsSliceEqual (util/signal/misc.go:22-35) when sym[] are
 *       action symbols (namazu_amd/historystorage.py).
 *   entity != NULL: partial-order mode, the reference default (-po-reduction=true, :42;
 *       createTracesPerEntity / tracesEqualInPO :62-124): entity[t] is the element's entity
 *       id, dense per trace (< 16384), NMZ_NONE for actions without an event (skipped);
 *       sym[] are event symbols (Event.Equals). Traces are equal iff every entity's projected
 *       subsequence is equal.
 * sig[2*n_traces]: 128-bit signature per trace (equal traces -> equal signatures; distinct
 * ones collide with probability ~2^-128). first_equal[i] = the smallest j with sig_j == sig_i
 * (j <= i), so the unique-trace curve of visualize is the running count of first_equal[i] == i.
 * Both refuse decreasing offsets (NMZ_EINVAL, "offsets must be non-decreasing"), before the context is looked at. */
int nmz_trace_signatures(nmz_ctx *ctx, const uint64_t *off, const uint64_t *sym, const uint32_t *entity,
                         uint32_t n_traces, uint64_t *sig);
int nmz_unique_traces(nmz_ctx *ctx, const uint64_t *off, const uint64_t *sym, const uint32_t *entity,
                      uint32_t n_traces, uint32_t *first_equal);
/* Device-resident variant: d_entity may be NULL (exact mode); entity ids must be < max_entities (<= 16384;
 * larger ids are skipped like NMZ_NONE, so the caller must pass the true bound);
 * d_sig[2*n_traces] receives the signatures. Enqueued on `stream` (NULL = the context's). */
int nmz_unique_traces_dev(nmz_ctx *ctx, const uint64_t *d_off, const uint64_t *d_sym, const uint32_t *d_entity,
                          uint32_t n_traces, uint32_t max_entities, uint64_t *d_sig, uint32_t *d_first_equal,
                          void *stream);

/* ---- replayable policy: delivery-order classes of seeds ---------------------
 * Replayable.QueueEvent releases every event at arrival + determineInterval(event)
 * (replayablepolicy.go:100-126), so a seed is a delivery order; `nmz tools visualize` classes runs by the equality
 * of their orders (cli/tools/visualize.go:51-136). These entry points join the two: which of N seeds deliver
 * distinct orders, which single seed to replay for each, and which orders the history already holds.
 * For one trace the caller gives the hints (CSR, n_events), arrival_ns[n_events], max_interval_ns, sym[n_events]
 * (uint64 event or action symbols, as nmz_trace_signatures takes them) and optionally entity[n_events] (uint32,
 * NMZ_NONE = skipped, as nmz_unique_traces; NULL = exact mode). For seed s:
 *     release[s][e] = arrival_ns[e] + delay[s][e]      (delay as nmz_replayable_sweep; 0 when max_interval_ns == 0)
 *     delivery order pi_s = the counted events sorted by (release asc, event index asc)
 *     rank[s][e]    = exact mode: position of e in pi_s
 *                     PO mode:    position of e among the events of its own entity in pi_s
 *     sig[s]        = the 128-bit signature nmz_trace_signatures gives the trace (sym[pi_s(0)], sym[pi_s(1)], ...)
 *                     with entity[pi_s(i)], bit for bit (the sum of the (symbol, rank) mixes plus the count terms;
 *                     entity id values are never read, only the ranks)
 *     gap           = release difference of two events consecutive in a compared sequence (the whole order in
 *                     exact mode, each entity's projection in PO mode)
 *     min_gap_ns[s] = the smallest gap (INT64_MAX when no pair is compared)
 *     gap_event[s]  = among the pairs attaining it, the smallest event index of the pair's later event
 *                     (NMZ_NONE when none)
 * Equal releases are a race in the reference (it sleeps in real time); the tie rule (event index) makes the order
 * deterministic and min_gap_ns == 0 reports the race. Because sig[s] equals the signature of a recorded run with
 * the same delivery, predicted and recorded signatures can be classed together (nmz_sig_classes_dev).
 * Limits, each NMZ_EINVAL with a message: 1 <= n_events <= NMZ_DELIVERY_MAX_EVENTS; 0 <= arrival_ns <= 2^50;
 * 0 <= max_interval_ns <= 2^50 (release * 4096 + e is then one 63-bit sort key with the tie rule built in);
 * entity ids < 16384 or NMZ_NONE; max_seeds < 2^32; hint offsets non-decreasing. Equal hints are legal. */
#define NMZ_DELIVERY_MAX_EVENTS 4096

/* Per-seed result of a delivery sweep, 32 bytes. */
typedef struct nmz_delivery_stats {
    uint64_t sig_lo;     /* the signature, as sig[2 i], sig[2 i + 1] of nmz_trace_signatures */
    uint64_t sig_hi;
    int64_t min_gap_ns;  /* smallest gap of the compared sequences; INT64_MAX when none      */
    uint32_t gap_event;  /* the later event of the first pair attaining it; NMZ_NONE if none */
    uint32_t n_counted;  /* events in the order (n_events minus the NMZ_NONE ones)           */
} nmz_delivery_stats;

/* One seed on the calling host thread, no device work (replayablepolicy.go:100-126; the signature's classes are
 * those of visualize.go:51-136): plain FNV-1a over seed || hint, a u64 remainder and a comparison sort, so it
 * checks the kernel's tables, reductions and sorting network independently. stats may be NULL. order (may be NULL)
 * receives the delivery order, n_counted event indices followed by NMZ_NONE up to n_events; release_ns (may be NULL)
 * every event's release. The only form that returns the permutation itself. */
int nmz_replayable_delivery_host(const uint8_t *seed, uint32_t seed_len, const uint32_t *hint_off,
                                 const uint8_t *hint_bytes, uint32_t n_events, int64_t max_interval_ns,
                                 const int64_t *arrival_ns, const uint64_t *sym, const uint32_t *entity,
                                 nmz_delivery_stats *stats, uint32_t *order, int64_t *release_ns);
/* The plan owns the device tables of one trace (grouped by entity) and the scratch of one sweep of up to max_seeds
 * (< 2^32) seeds; host arrays are borrowed for the call. It serves one stream at a time; destroy waits for the
 * plan's sweeps (replayablepolicy.go:100-126). */
typedef struct nmz_replayable_delivery_plan nmz_replayable_delivery_plan;
int nmz_replayable_delivery_plan_create(nmz_ctx *ctx, const uint32_t *hint_off, const uint8_t *hint_bytes,
                                        uint32_t n_events, int64_t max_interval_ns, const int64_t *arrival_ns,
                                        const uint64_t *sym, const uint32_t *entity /* may be NULL */,
                                        uint64_t max_seeds, nmz_replayable_delivery_plan **out);
int nmz_replayable_delivery_plan_destroy(nmz_replayable_delivery_plan *plan);
/* d_stats[n_seeds] for the seeds "seed_lo" .. "seed_lo + n_seeds - 1" (decimal strings generated on the device,
 * wrapping past 2^64; replayablepolicy.go:74-87 seed string, :100-126 release times), enqueued on `stream`
 * (NULL = the context's). */
int nmz_replayable_delivery_sweep_decimal_dev(nmz_replayable_delivery_plan *plan, uint64_t seed_lo, uint64_t n_seeds,
                                              nmz_delivery_stats *d_stats, void *stream);
/* The same for arbitrary seed strings (device CSR d_seed_off[n_seeds + 1] into d_seed_bytes; the empty seed is the
 * reference's default, replayablepolicy.go:74-81, :100-126). */
int nmz_replayable_delivery_sweep_dev(nmz_replayable_delivery_plan *plan, const uint32_t *d_seed_off,
                                      const uint8_t *d_seed_bytes, uint64_t n_seeds, nmz_delivery_stats *d_stats,
                                      void *stream);
/* Classes over the stats of a sweep (visualize.go:51-136 equality, on predicted orders): d_first_equal[n] = the
 * smallest j with an equal signature; d_class_rep[n] (may be NULL) = for a class head h (first_equal[h] == h) the
 * member with the largest min_gap_ns, ties to the smallest index, the seed to replay for that order, and NMZ_NONE
 * for every other i; *d_n_classes (may be NULL) = the number of classes. n < 2^31. Enqueued on `stream` (NULL =
 * the context's); scratch is the context's, so one call at a time per context. */
int nmz_delivery_classes_dev(nmz_ctx *ctx, const nmz_delivery_stats *d_stats, uint32_t n, uint32_t *d_first_equal,
                             uint32_t *d_class_rep, uint32_t *d_n_classes, void *stream);
/* The plain form over d_sig[2 n] (visualize.go:51-136): signatures of recorded runs (nmz_trace_signatures) and
 * predicted ones (the stats' sig_lo, sig_hi) in one array are classed together. */
int nmz_sig_classes_dev(nmz_ctx *ctx, const uint64_t *d_sig, uint32_t n, uint32_t *d_first_equal, void *stream);
/* Host pointers, synchronous: plan + sweep + classes (replayablepolicy.go:100-126, visualize.go:51-136).
 * stats[n_seeds], first_equal[n_seeds], class_rep[n_seeds] and n_classes may each be NULL. */
int nmz_replayable_delivery_sweep(nmz_ctx *ctx, const uint32_t *seed_off, const uint8_t *seed_bytes, uint64_t n_seeds,
                                  const uint32_t *hint_off, const uint8_t *hint_bytes, uint32_t n_events,
                                  int64_t max_interval_ns, const int64_t *arrival_ns, const uint64_t *sym,
                                  const uint32_t *entity, nmz_delivery_stats *stats, uint32_t *first_equal,
                                  uint32_t *class_rep, uint32_t *n_classes);
int nmz_replayable_delivery_sweep_decimal(nmz_ctx *ctx, uint64_t seed_lo, uint64_t n_seeds, const uint32_t *hint_off,
                                          const uint8_t *hint_bytes, uint32_t n_events, int64_t max_interval_ns,
                                          const int64_t *arrival_ns, const uint64_t *sym, const uint32_t *entity,
                                          nmz_delivery_stats *stats, uint32_t *first_equal, uint32_t *class_rep,
                                          uint32_t *n_classes);

/* ---- replayable policy: seeds nearest to a recorded delivery order -----------
 * A recorded failing run usually has no seed (the random policy reseeds from the clock, util/queue/impl.go:39);
 * the replayable policy reproduces a run only from a known seed (replayablepolicy.go:63-126). These entry points
 * answer: among N replayable seeds, which deliver the events in the order nearest to the recorded one?
 * For one trace the caller gives the hints (CSR, n_events), arrival_ns[n_events] and max_interval_ns as the
 * delivery sweep takes them, optionally entity[n_events] (NULL = exact mode, NMZ_NONE = skipped), and
 * target_pos[n_events] (uint32): the event's position in the recorded order, NMZ_NONE if the recorded run does not
 * contain it. An event is counted iff target_pos != NMZ_NONE and, in PO mode, entity != NMZ_NONE. The target_pos
 * of counted events must be distinct; they need not be dense (only their order is read).
 * Releases, the delivery order pi_s of the counted events (release asc, event index asc) and the compared sequences
 * (the whole order in exact mode, each entity's projection in PO mode) are the delivery sweep's above. For seed s:
 *     n_discordant = #{(a, b) in one compared sequence : target_pos[a] < target_pos[b] and b precedes a in pi_s}
 *                    (Kendall tau distance; PO mode counts same-entity pairs only, the pairs tracesEqualInPO sees)
 *     in place     = event e's rank in its compared sequence in pi_s equals its rank there by target_pos
 *     prefix_len   = how many leading events of the target order (counted events by target_pos ascending) are all
 *                    in place: the common prefix of pi_s and the target (exact), the longest target prefix every
 *                    entity sees unchanged (PO); the notion of HistoryStorage.Search(prefix),
 *                    historystorage/naive/naive.go:235-257. Equals n_counted when the orders match.
 *     min_gap_ns, gap_event = as nmz_delivery_stats, over the counted events
 *     n_in_place   = events in place
 * n_discordant == 0 <=> every compared sequence is in target order <=> the seed's delivery signature
 * (nmz_delivery_stats over the same counted events) equals the recorded run's.
 * The plan reports n_counted and n_pairs = the sum over the compared sequences of n (n - 1) / 2 (<= 8,386,560).
 * Ranking is written as nmz_topk_entry (sentinel and .seed as the order sweep's lists, so nmz_topk_merge_dev and
 * namazu_amd/replay.py serve it unchanged):
 *     NMZ_TARGET_RANK_PAIRS:  n_fault = n_pairs - n_discordant, sum_delay_ns = min_gap_ns, first_fault = prefix_len
 *     NMZ_TARGET_RANK_PREFIX: n_fault = prefix_len, sum_delay_ns = n_pairs - n_discordant, first_fault = n_in_place
 * Limits, each NMZ_EINVAL with a message: those of the delivery sweep (1 <= n_events <= 4096; arrivals and
 * max_interval_ns in [0, 2^50]; entity ids < 16384 or NMZ_NONE; max_seeds < 2^32; hint offsets non-decreasing);
 * a target_pos that appears twice among the counted events; an unknown rank mode. With nothing counted or
 * max_interval_ns == 0 every seed has the same record. */
#define NMZ_TARGET_RANK_PAIRS 0
#define NMZ_TARGET_RANK_PREFIX 1

/* Per-seed result of a nearest-order sweep, 24 bytes. */
typedef struct nmz_target_stats {
    uint32_t n_discordant; /* pairs delivered the other way round than the target orders them */
    uint32_t prefix_len;   /* leading events of the target order that are all in place         */
    int64_t min_gap_ns;    /* smallest gap of the compared sequences; INT64_MAX when none      */
    uint32_t gap_event;    /* the later event of the first pair attaining it; NMZ_NONE if none */
    uint32_t n_in_place;   /* events whose rank equals their target rank                       */
} nmz_target_stats;

/* One seed on the calling host thread, no device work (replayablepolicy.go:100-126 release times;
 * historystorage/naive/naive.go:235-257 the prefix): plain FNV-1a over seed || hint, a u64 remainder, a comparison
 * sort and a merge count per sequence; it shares no table or reduction with the kernel. stats, n_counted and
 * n_pairs may each be NULL. Vets a candidate seed before a replay. */
int nmz_replayable_target_host(const uint8_t *seed, uint32_t seed_len, const uint32_t *hint_off,
                               const uint8_t *hint_bytes, uint32_t n_events, int64_t max_interval_ns,
                               const int64_t *arrival_ns, const uint32_t *entity /* may be NULL */,
                               const uint32_t *target_pos, nmz_target_stats *stats, uint32_t *n_counted,
                               uint32_t *n_pairs);
/* The plan owns the device tables of one trace and target and the scratch of one sweep of up to max_seeds (< 2^32)
 * seeds; host arrays are borrowed for the call. It serves one stream at a time; destroy waits for the plan's sweeps
 * (replayablepolicy.go:100-126, historystorage/naive/naive.go:235-257). */
typedef struct nmz_replayable_target_plan nmz_replayable_target_plan;
int nmz_replayable_target_plan_create(nmz_ctx *ctx, const uint32_t *hint_off, const uint8_t *hint_bytes,
                                      uint32_t n_events, int64_t max_interval_ns, const int64_t *arrival_ns,
                                      const uint32_t *entity /* may be NULL */, const uint32_t *target_pos,
                                      uint64_t max_seeds, nmz_replayable_target_plan **out);
int nmz_replayable_target_plan_destroy(nmz_replayable_target_plan *plan);
/* The plan's constants (replayablepolicy.go:100-126, naive.go:235-257): each pointer may be NULL. */
int nmz_replayable_target_plan_info(const nmz_replayable_target_plan *plan, uint32_t *n_counted, uint32_t *n_pairs);
/* The seeds "seed_lo" .. "seed_lo + n_seeds - 1" (decimal strings generated on the device, wrapping past 2^64;
 * replayablepolicy.go:74-87 seed string, :100-126 release times; naive.go:235-257), enqueued on `stream` (NULL = the
 * context's). d_stats[n_seeds] may be NULL: the sweep then writes only d_topk[k] (k <= 256; k == 0: no top-k).
 * Top-k .seed = the seed's integer value. */
int nmz_replayable_target_sweep_decimal_dev(nmz_replayable_target_plan *plan, uint64_t seed_lo, uint64_t n_seeds,
                                            int rank_mode, uint32_t k, nmz_target_stats *d_stats /* may be NULL */,
                                            nmz_topk_entry *d_topk, void *stream);
/* The same for arbitrary seed strings (device CSR d_seed_off[n_seeds + 1] into d_seed_bytes; the empty seed is the
 * reference's default, replayablepolicy.go:74-81, :100-126; naive.go:235-257). Top-k .seed = seed0 + the seed's
 * index. */
int nmz_replayable_target_sweep_dev(nmz_replayable_target_plan *plan, const uint32_t *d_seed_off,
                                    const uint8_t *d_seed_bytes, uint64_t n_seeds, uint64_t seed0, int rank_mode,
                                    uint32_t k, nmz_target_stats *d_stats /* may be NULL */, nmz_topk_entry *d_topk,
                                    void *stream);
/* Host pointers, synchronous: plan + sweep + top-k (replayablepolicy.go:100-126, naive.go:235-257). stats[n_seeds],
 * topk[k] (k <= 256), n_counted and n_pairs may each be NULL. Top-k .seed = the seed's index in the CSR, or its
 * integer value for the decimal form. */
int nmz_replayable_target_sweep(nmz_ctx *ctx, const uint32_t *seed_off, const uint8_t *seed_bytes, uint64_t n_seeds,
                                const uint32_t *hint_off, const uint8_t *hint_bytes, uint32_t n_events,
                                int64_t max_interval_ns, const int64_t *arrival_ns, const uint32_t *entity,
                                const uint32_t *target_pos, int rank_mode, uint32_t k, nmz_target_stats *stats,
                                nmz_topk_entry *topk, uint32_t *n_counted, uint32_t *n_pairs);
int nmz_replayable_target_sweep_decimal(nmz_ctx *ctx, uint64_t seed_lo, uint64_t n_seeds, const uint32_t *hint_off,
                                        const uint8_t *hint_bytes, uint32_t n_events, int64_t max_interval_ns,
                                        const int64_t *arrival_ns, const uint32_t *entity, const uint32_t *target_pos,
                                        int rank_mode, uint32_t k, nmz_target_stats *stats, nmz_topk_entry *topk,
                                        uint32_t *n_counted, uint32_t *n_pairs);

/* ---- order contrast: the event pairs whose order separates failing runs from passing ones ------------
 * A history storage holds many recorded runs, each labelled by its result.json (IsSuccessful,
 * historystorage/naive/naive.go:199-213; `nmz tools summary` prints the failing ones, cli/tools/summary.go:40-57).
 * These entry points answer: which few ordered event pairs are released one way round in the failing runs and the
 * other way round in the passing ones? Those pairs are the constraints nmz_replayable_order_sweep* takes.
 * For one event universe (the trace whose hints the sweeps take) the caller gives
 *     pos[n_runs][n_events]  uint32, row-major: the position of event e in recorded run r, NMZ_NONE if the run does
 *                            not hold it; any other value is legal and positions need not be dense (one
 *                            match_target row per run, namazu_amd/historystorage.py)
 *     failed[n_runs]         uint8, 1 = the run failed, 0 = it passed.
 * With n_fail and n_pass the numbers of failing and passing runs, for every ordered pair (b, a), b != a:
 *     F(b,a) = #{failing r : pos[r][b] != NONE, pos[r][a] != NONE, pos[r][b] < pos[r][a]}
 *     P(b,a) = the same over the passing runs
 *     score(b,a) = F(b,a) * n_pass - P(b,a) * n_fail        (int64; = n_fail n_pass (F / n_fail - P / n_pass))
 * Two events at equal positions in a run count for neither direction. Pairs are ranked by (score desc, F desc,
 * b * n_events + a asc), a strict total order; only pairs with score > 0 are listed, and past them the list holds
 * the sentinel {NMZ_NONE, NMZ_NONE, INT64_MIN, 0, 0, 0, 0}. n_positive is the number of ordered pairs with score > 0.
 * Limits, each NMZ_EINVAL with a message: 1 <= n_events <= NMZ_DELIVERY_MAX_EVENTS; 1 <= n_runs <=
 * NMZ_CONTRAST_MAX_RUNS (two 16-bit counts pack into one word, n_fail n_pass < 2^32, every score fits int64 with
 * INT64_MIN free); failed[r] in {0, 1}; at least one failing and one passing run; k <= 256. */
#define NMZ_CONTRAST_MAX_RUNS 65535

/* One listed pair, 32 bytes: failing runs release `before` ahead of `after`. */
typedef struct nmz_order_pair {
    uint32_t before, after;
    int64_t score;
    uint32_t n_fail_with, n_pass_with;       /* F(before, after), P(before, after) */
    uint32_t n_fail_against, n_pass_against; /* F(after, before), P(after, before) */
} nmz_order_pair;
/* Counts of one ordered pair, at [b * n_events + a]; the diagonal is 0. */
typedef struct nmz_pair_counts {
    uint32_t n_fail_with, n_pass_with;
} nmz_pair_counts;
typedef struct nmz_contrast_info {
    uint32_t n_fail, n_pass;
    uint64_t n_positive;
} nmz_contrast_info;

/* One pair on the calling host thread, no device work (naive.go:199-213 IsSuccessful, cli/tools/summary.go:40-57):
 * plain loops over the runs by the definition above; it shares no code with the kernels. Checks every limit above
 * and before != after, both < n_events. out and info may each be NULL; info->n_positive is 0 (one pair says nothing
 * about the others). Serves the CPU tests, and vets a pair before hours of replays are spent on it. */
int nmz_order_contrast_host(const uint32_t *pos, const uint8_t *failed, uint32_t n_runs, uint32_t n_events,
                            uint32_t before, uint32_t after, nmz_order_pair *out, nmz_contrast_info *info);
/* Device pointers, enqueued on `stream` (NULL = the context's); scratch from the context, which serves one contrast
 * at a time (naive.go:199-213, cli/tools/summary.go:40-57). d_counts[n_events * n_events] may be NULL: nothing of
 * size n_events^2 is then written or allocated (the hot form). d_pairs[k] (k <= 256; k == 0: no list) and d_info are
 * written on the stream. The sizes and k are checked before any launch; the labels are on the device and are not
 * read by the host: any nonzero label counts as failing, and with no failing or no passing run every score is 0,
 * the list is all sentinels and n_positive is 0 (d_info still reports n_fail and n_pass). */
int nmz_order_contrast_dev(nmz_ctx *ctx, const uint32_t *d_pos, const uint8_t *d_failed, uint32_t n_runs,
                           uint32_t n_events, uint32_t k, nmz_pair_counts *d_counts /* may be NULL */,
                           nmz_order_pair *d_pairs, nmz_contrast_info *d_info, void *stream);
/* Host pointers, synchronous, built on the _dev form (naive.go:199-213, cli/tools/summary.go:40-57). Every limit
 * above, the labels included, is checked before any device work. counts, pairs and info may each be NULL. */
int nmz_order_contrast(nmz_ctx *ctx, const uint32_t *pos, const uint8_t *failed, uint32_t n_runs, uint32_t n_events,
                       uint32_t k, nmz_pair_counts *counts /* may be NULL */, nmz_order_pair *pairs,
                       nmz_contrast_info *info);

/* ---- matching stored runs to the event universe: pos[n_runs][n_events] made on the device ------------------
 * The reference walks its stored runs one by one (historystorage/naive/naive.go:235-257), each handed out by
 * GetStoredHistory (historystorage/historystorage.go:45). These entry points turn the runs' symbol sequences into
 * the pos array nmz_order_contrast* takes (and, one row, the target_pos of nmz_replayable_target_*), by the rule of
 * match_target (namazu_amd/historystorage.py):
 *     the universe is sym[n_events] (uint64) with arrival_ns[n_events] (int64);
 *     the events carrying one symbol value are ordered by (arrival asc, event index asc), and occurrence j of that
 *     order is "the j-th event with the symbol";
 *     run r is the symbol slice run_sym[run_off[r] .. run_off[r + 1]);
 *     the i-th occurrence of a value in the run (counting from 0 in run order), at run position p, is matched to the
 *     i-th event with that value: pos[r][e] = p;
 *     events without a matched occurrence get NMZ_NONE; run elements whose value is not in the universe, and
 *     occurrences beyond the universe's count of that value, are ignored. Positions are indexes into the run, so a
 *     row can have holes.
 * Limits of the host forms, each NMZ_EINVAL with a message, checked before any device work: 1 <= n_events <=
 * NMZ_DELIVERY_MAX_EVENTS; run_off[0] == 0 and the offsets non-decreasing; every run shorter than 2^32 - 1
 * elements (NMZ_NONE stays free); n_runs * n_events fits the output. n_runs == 0 is legal and writes nothing. */

/* One run on the calling host thread, no device work (naive.go:235-257, historystorage.go:45 GetStoredHistory):
 * plain loops by the definition (a stable sort of the events by arrival, then for each run element the first
 * unmatched event with its symbol); it shares no table or reduction with the kernel. pos[n_events]. */
int nmz_match_run_host(const uint64_t *sym, const int64_t *arrival_ns, uint32_t n_events, const uint64_t *run_sym,
                       uint64_t run_len, uint32_t *pos);
/* The plan owns the universe's device tables (naive.go:235-257, historystorage.go:45 GetStoredHistory): the distinct
 * symbols, each symbol's event list in (arrival, index) order, and the counts. Host arrays are borrowed for the
 * call. A plan serves any number of matches on any streams; destroy waits for them. */
typedef struct nmz_match_plan nmz_match_plan;
int nmz_match_plan_create(nmz_ctx *ctx, const uint64_t *sym, const int64_t *arrival_ns, uint32_t n_events,
                          nmz_match_plan **out);
int nmz_match_plan_destroy(nmz_match_plan *plan);
/* The plan's constants (naive.go:235-257, historystorage.go:45 GetStoredHistory): n_symbols = the number of distinct
 * symbols; each pointer may be NULL. */
int nmz_match_plan_info(const nmz_match_plan *plan, uint32_t *n_events, uint32_t *n_symbols);
/* Device CSR in (naive.go:235-257, historystorage.go:45 GetStoredHistory): d_run_off[n_runs + 1] and d_run_sym, both
 * uint64, the layout nmz_unique_traces_dev takes; row-major uint32 d_pos[n_runs][n_events] out, the array
 * nmz_order_contrast_dev takes and, one row, a target_pos. Enqueued on `stream` (NULL = the context's). The host
 * cannot read the offsets: they must be non-decreasing and stay inside d_run_sym (a decreasing pair reads as an
 * empty run), and elements at run positions >= 2^32 - 1 are ignored. */
int nmz_match_runs_dev(nmz_match_plan *plan, const uint64_t *d_run_off, const uint64_t *d_run_sym, uint64_t n_runs,
                       uint32_t *d_pos, void *stream);
/* Host pointers, synchronous, built on the _dev form (naive.go:235-257, historystorage.go:45 GetStoredHistory):
 * plan + upload + match + pos[n_runs][n_events] back. The device buffers are taken for the call from the context's
 * pool. */
int nmz_match_runs(nmz_ctx *ctx, const uint64_t *sym, const int64_t *arrival_ns, uint32_t n_events,
                   const uint64_t *run_off, const uint64_t *run_sym, uint64_t n_runs, uint32_t *pos);
/* nmz_order_contrast from the stored runs themselves (naive.go:235-257, historystorage.go:45 GetStoredHistory; the
 * labels naive.go:199-213): host pointers, synchronous. The CSR is uploaded, matched on the device and fed to
 * nmz_order_contrast_dev; pos never leaves the device. Its [n_runs][n_events] rows (up to 1 GB) are taken for the
 * call from the context's pool, not from the contrast's fixed scratch. Every limit and label check of
 * nmz_order_contrast and of nmz_match_runs holds, with the same messages, before any device work. counts, pairs and
 * info may each be NULL. The results are byte-identical to nmz_order_contrast over nmz_match_runs' output. */
int nmz_order_contrast_runs(nmz_ctx *ctx, const uint64_t *sym, const int64_t *arrival_ns, uint32_t n_events,
                            const uint64_t *run_off, const uint64_t *run_sym, const uint8_t *failed, uint32_t n_runs,
                            uint32_t k, nmz_pair_counts *counts /* may be NULL */, nmz_order_pair *pairs,
                            nmz_contrast_info *info);

/* ---- edit scripts for trace pairs: what differs between two stored runs ------------------------------------
 * A build-defined extension of the optional similarity interface (historystorage/historystorage.go:50-51); the
 * reference has equality only (naive/naive.go:235-257), and an empty script <=> SingleTrace.Equals
 * (util/trace/trace.go:29-31). For traces a (n symbols) and b (m symbols) and a band w:
 *     dist = ED_w(a, b) = min(Lev(a, b), w + 1), exactly nmz_ed_pairs' value; dist == w + 1: no script;
 *     otherwise the script is the canonical optimal alignment over the unit-cost Levenshtein matrix D: walk back
 *     from (n, m) to (0, 0) taking at (i, j) the first move that applies --
 *       1. diagonal: i, j > 0 and D[i-1][j-1] + (a[i-1] != b[j-1]) == D[i][j]: a match (no op) or NMZ_EDIT_SUB;
 *       2. up: i > 0 and D[i-1][j] + 1 == D[i][j]: NMZ_EDIT_DEL;
 *       3. left otherwise: NMZ_EDIT_INS;
 *     the ops in forward order, matches omitted: exactly dist ops. a_pos / b_pos are the numbers of elements of a
 *     and b consumed before the op. The script turns a into b; script(b, a) need not mirror it.
 * Output per pair: `band` slots, the ops, then {NMZ_NONE, NMZ_NONE, NMZ_NONE}. Pair (ia, ib) aligns a = trace ia to
 * b = trace ib. Limits, each NMZ_EINVAL with a message, checked before any device work (arguments before the
 * context): band <= NMZ_ALIGN_MAX_BAND (wider bands are not built yet); traces shorter than 2^32 - 1 elements; pair
 * indexes < n_traces; offsets non-decreasing. n_pairs == 0 is legal and needs no device; band == 0 is legal (dist in
 * {0, 1}, ops may be NULL). */
#define NMZ_ALIGN_MAX_BAND 64
#define NMZ_EDIT_SUB 0u /* a[a_pos] becomes b[b_pos]                                  */
#define NMZ_EDIT_DEL 1u /* a[a_pos] is dropped                                        */
#define NMZ_EDIT_INS 2u /* b[b_pos] is inserted before a[a_pos]; a_pos may be n       */
typedef struct nmz_edit_op {
    uint32_t a_pos;
    uint32_t b_pos;
    uint32_t kind;
} nmz_edit_op;
/* One pair on the calling host thread, no device work (historystorage.go:50-51, naive.go:235-257,
 * util/trace/trace.go:29-31): a plain +inf-banded DP that keeps its band rows, then the walk above. It shares no
 * table or reduction with the kernel: the form to vet a script with, and the check of the device forms. */
int nmz_ed_align_host(const uint64_t *a, uint64_t n, const uint64_t *b, uint64_t m, uint32_t band,
                      uint32_t *dist, nmz_edit_op *ops /* [band] */);
/* The plan owns the history scratch (historystorage.go:50-51, naive.go:235-257, util/trace/trace.go:29-31): 2 bits
 * per band cell and row, for `slots` pairs in flight of up to max_len elements each, 256 MiB at the most in all. A
 * max_len whose single pair exceeds that is NMZ_EINVAL. The plan serves one stream at a time (a launch on another
 * stream waits for the one before); destroy waits for its launches. */
typedef struct nmz_ed_align_plan nmz_ed_align_plan;
int nmz_ed_align_plan_create(nmz_ctx *ctx, uint32_t band, uint64_t max_len, nmz_ed_align_plan **out);
int nmz_ed_align_plan_destroy(nmz_ed_align_plan *plan);
/* The plan's constants (historystorage.go:50-51, naive.go:235-257, util/trace/trace.go:29-31): the pairs in flight
 * and the bytes of history scratch behind them; each pointer may be NULL. */
int nmz_ed_align_plan_info(const nmz_ed_align_plan *plan, uint32_t *slots, uint64_t *history_bytes);
/* Device CSR and device pairs in, d_dist[n_pairs] and d_ops[n_pairs * band] out (historystorage.go:50-51,
 * naive.go:235-257, util/trace/trace.go:29-31); enqueued on `stream` (NULL = the context's), nothing else. The host
 * cannot read the offsets: they must be non-decreasing and stay inside d_sym, the pair indexes below the number of
 * traces (a decreasing pair of offsets reads as an empty trace), and a pair with a trace longer than the plan's
 * max_len gets dist = NMZ_NONE and sentinel ops. */
int nmz_ed_align_pairs_dev(nmz_ed_align_plan *plan, const uint64_t *d_off, const uint64_t *d_sym,
                           const uint32_t *d_pairs, uint64_t n_pairs, uint32_t *d_dist,
                           nmz_edit_op *d_ops /* [n_pairs * band] */, void *stream);
/* Host pointers, synchronous, built on the _dev form (historystorage.go:50-51, naive.go:235-257,
 * util/trace/trace.go:29-31): a plan for the longest trace of the pairs given + upload + launch + download. The
 * device buffers are taken for the call from the context's pool. pairs[2 * n_pairs], dist[n_pairs],
 * ops[n_pairs * band]. */
int nmz_ed_align_pairs(nmz_ctx *ctx, const uint64_t *off, const uint64_t *sym, uint32_t n_traces,
                       const uint32_t *pairs, uint64_t n_pairs, uint32_t band, uint32_t *dist, nmz_edit_op *ops);

/* ---- edit scripts over wider bands: 0 <= band <= NMZ_ALIGN_WIDE_MAX_BAND ------------------------------------
 * The same build-defined extension (historystorage/historystorage.go:50-51; the reference has equality only,
 * naive/naive.go:235-257; util/trace/trace.go:29-31), with the semantics above word for word: dist = min(Lev, band +
 * 1), the canonical alignment for dist <= band, `band` slots per pair, sentinels behind the ops, nmz_edit_op as it
 * is. The script does not depend on the band once Lev <= band, so a pair with Lev <= 64 gets at any wide band the ops
 * that the narrow form gives at band 64. Every band 0 .. 1024 is accepted: for band <= NMZ_ALIGN_MAX_BAND these
 * entry points return byte for byte what their narrow counterparts return (they run the same kernel), beyond it
 * k_ed_align_wide does the work. Limits, each NMZ_EINVAL with a message, checked before any device work (arguments
 * before the context): band <= NMZ_ALIGN_WIDE_MAX_BAND (wider bands are not built yet); traces shorter than 2^32 - 1
 * elements; pair indexes < n_traces; offsets non-decreasing; n_pairs * band fits the output. n_pairs == 0 is legal
 * and needs no device; band == 0 is legal (ops may be NULL). The nmz_ed_align_*, nmz_move_profile{_host, _dev,} and
 * nmz_ed_diff_profile entry points keep NMZ_ALIGN_MAX_BAND; nmz_move_profile_wide* and nmz_ed_diff_profile_wide
 * (below) tally these scripts. */
#define NMZ_ALIGN_WIDE_MAX_BAND 1024
/* One pair on the calling host thread, no device work (historystorage.go:50-51, naive.go:235-257,
 * util/trace/trace.go:29-31): nmz_ed_align_host's plain +inf-banded DP with 16-bit cells (they hold band + 1 <=
 * 1025), its band rows kept whole -- (n + 1) * (2 band + 1) * 2 bytes, NMZ_ENOMEM with the sizes when they do not
 * fit -- then the walk by the definition. It shares no table, scan or packed history with the kernels: the check of
 * the device forms. */
int nmz_ed_align_wide_host(const uint64_t *a, uint64_t n, const uint64_t *b, uint64_t m, uint32_t band,
                           uint32_t *dist, nmz_edit_op *ops /* [band] */);
/* The plan owns the history scratch (historystorage.go:50-51, naive.go:235-257, util/trace/trace.go:29-31): 2 bits
 * per band cell and row (the band's cells rounded up to 256 * {1, 2, 3, 5, 9}: 64 .. 576 bytes per row), for `slots`
 * pairs in flight of up to max_len elements each, 256 MiB at the most in all -- at band 1024 about 466,000 rows. A
 * max_len whose single pair exceeds that is NMZ_EINVAL naming both numbers. The plan serves one stream at a time (a
 * launch on another stream waits for the one before); destroy waits for its launches. */
typedef struct nmz_ed_align_wide_plan nmz_ed_align_wide_plan;
int nmz_ed_align_wide_plan_create(nmz_ctx *ctx, uint32_t band, uint64_t max_len, nmz_ed_align_wide_plan **out);
int nmz_ed_align_wide_plan_destroy(nmz_ed_align_wide_plan *plan);
/* The plan's constants (historystorage.go:50-51, naive.go:235-257, util/trace/trace.go:29-31): the pairs in flight
 * and the bytes of history scratch behind them; each pointer may be NULL. */
int nmz_ed_align_wide_plan_info(const nmz_ed_align_wide_plan *plan, uint32_t *slots, uint64_t *history_bytes);
/* Device CSR and device pairs in, d_dist[n_pairs] and d_ops[n_pairs * band] out (historystorage.go:50-51,
 * naive.go:235-257, util/trace/trace.go:29-31); one launch enqueued on `stream` (NULL = the context's), nothing
 * else. The host cannot read the offsets: they must be non-decreasing and stay inside d_sym, the pair indexes below
 * the number of traces (a decreasing pair of offsets reads as an empty trace), and a pair with a trace longer than
 * the plan's max_len gets dist = NMZ_NONE and sentinel ops. */
int nmz_ed_align_wide_pairs_dev(nmz_ed_align_wide_plan *plan, const uint64_t *d_off, const uint64_t *d_sym,
                                const uint32_t *d_pairs, uint64_t n_pairs, uint32_t *d_dist,
                                nmz_edit_op *d_ops /* [n_pairs * band] */, void *stream);
/* Host pointers, synchronous, built on the _dev form (historystorage.go:50-51, naive.go:235-257,
 * util/trace/trace.go:29-31): a plan for the longest trace of the pairs given + upload + launch + download. The
 * device buffers are taken for the call from the context's pool. pairs[2 * n_pairs], dist[n_pairs],
 * ops[n_pairs * band]. */
int nmz_ed_align_wide_pairs(nmz_ctx *ctx, const uint64_t *off, const uint64_t *sym, uint32_t n_traces,
                            const uint32_t *pairs, uint64_t n_pairs, uint32_t band, uint32_t *dist, nmz_edit_op *ops);

/* ---- move profiles: which events move between the runs of many pairs ----------------------------------------
 * A build-defined extension of the same optional interface (historystorage/historystorage.go:50-51; the reference has
 * equality only, naive/naive.go:235-257; the labels of failing and passing runs naive.go:199-213). Input: the scripts
 * nmz_ed_align_* gives, `band` slots per pair and dist per pair. A pair with dist <= band is a *script* of dist ops
 * o_0 .. o_{dist-1}; every other pair (dist == band + 1, dist == NMZ_NONE) is *beyond* and contributes nothing.
 *   Names.    A DEL names a[a_pos]. An INS names b[b_pos]. A SUB names a[a_pos] (from) and b[b_pos] (to).
 *   Partners. The r-th DEL naming value v (r from 0, script order) and the r-th INS naming v are partners: a *move*
 *             of v. partner[s] is the partner's slot index; NMZ_NONE for a DEL or INS without a partner, for every
 *             SUB, for sentinel slots and for every slot of a pair beyond the band.
 *   Direction. A move is *later* when its INS slot comes after its DEL slot (in b the event is delivered later than
 *             in a), else *earlier*; slots are strictly ordered, so there is no tie.
 *             span = |ops[ins].b_pos - ops[del].b_pos|.
 *   Profile.  usym[n_usym]: the symbols to tally, strictly increasing; n_usym == 0 is legal. counts[n_usym], one
 *             nmz_move_counts per table symbol; a name that is not in the table is skipped in the counters (it
 *             counts in info.n_unknown) but still pairs up in `partner`.
 * Limits of the host-pointer forms, each NMZ_EINVAL with a message, checked before any device work (arguments before
 * the context): everything nmz_ed_align_pairs checks, with its messages; usym strictly increasing;
 * n_pairs * band < 2^32 (no uint32 counter can wrap); where ops are an input, for the first dist slots of every
 * script: kind <= 2, a_pos < n for DEL / SUB, b_pos < m for INS / SUB. n_pairs == 0 is legal and needs no device:
 * the counters and the info are zero. */
typedef struct nmz_move_counts {
    uint32_t later;        /* moves of the symbol whose INS slot follows its DEL slot                     */
    uint32_t earlier;      /* moves of the symbol whose INS slot precedes its DEL slot                    */
    uint32_t dropped;      /* DELs of the symbol without a partner                                        */
    uint32_t extra;        /* INSs of the symbol without a partner                                        */
    uint32_t sub_from;     /* SUBs that name the symbol as a[a_pos]                                       */
    uint32_t sub_to;       /* SUBs that name the symbol as b[b_pos]                                       */
    uint32_t n_pairs;      /* scripts in which at least one op names the symbol (once per script)         */
    uint32_t reserved;     /* always 0                                                                    */
    uint64_t span_later;   /* sum of span over the symbol's later moves                                   */
    uint64_t span_earlier; /* sum of span over the symbol's earlier moves                                 */
} nmz_move_counts;
typedef struct nmz_move_info {
    uint64_t n_scripts; /* pairs with dist <= band                                                        */
    uint64_t n_beyond;  /* all other pairs                                                                */
    uint64_t n_ops;     /* sum of dist over the scripts                                                   */
    uint64_t n_unknown; /* names of ops that are not in the table (a SUB can add 2)                       */
} nmz_move_info;
/* One script on the calling host thread, no device work (historystorage.go:50-51, naive.go:235-257): partner[n_ops]
 * by the definition -- plain loops and a std::map of per-value queues. It shares nothing with the kernel: the form
 * to vet a result with. Every op is live: kind <= 2 and the positions it reads inside a / b, else NMZ_EINVAL. */
int nmz_script_moves_host(const uint64_t *a, uint64_t n, const uint64_t *b, uint64_t m, const nmz_edit_op *ops,
                          uint32_t n_ops, uint32_t *partner /* [n_ops] */);
/* The whole profile on the calling host thread, plain loops, no device work (historystorage.go:50-51,
 * naive.go:199-213, 235-257): for callers without a device, and the check of the device forms. dist[n_pairs] and
 * ops[n_pairs * band] as nmz_ed_align_pairs writes them; partner[n_pairs * band] may be NULL. */
int nmz_move_profile_host(const uint64_t *off, const uint64_t *sym, uint32_t n_traces, const uint32_t *pairs,
                          uint64_t n_pairs, uint32_t band, const uint32_t *dist, const nmz_edit_op *ops,
                          const uint64_t *usym, uint64_t n_usym, uint32_t *partner /* may be NULL */,
                          nmz_move_counts *counts /* [n_usym] */, nmz_move_info *info);
/* Device pointers in and out (historystorage.go:50-51, naive.go:199-213, 235-257); enqueued on `stream` (NULL = the
 * context's). accumulate == 0: d_counts[n_usym] and d_info are cleared on that stream first; accumulate != 0: the
 * call adds to them, so the batches of one job sum. Apart from the clear it enqueues one launch and allocates
 * nothing. The host cannot read the inputs: band <= NMZ_ALIGN_MAX_BAND, n_pairs * band < 2^32 and d_usym strictly
 * increasing are the caller's to keep, offsets and pairs as for nmz_ed_align_pairs_dev; an op of a script with
 * kind > 2 or a position outside its trace counts for nothing (no name, no partner), and the kernel makes no
 * out-of-range read for it. d_partner[n_pairs * band] may be NULL. */
int nmz_move_profile_dev(nmz_ctx *ctx, const uint64_t *d_off, const uint64_t *d_sym, const uint32_t *d_pairs,
                         uint64_t n_pairs, uint32_t band, const uint32_t *d_dist, const nmz_edit_op *d_ops,
                         const uint64_t *d_usym, uint64_t n_usym, uint32_t *d_partner /* may be NULL */,
                         nmz_move_counts *d_counts, nmz_move_info *d_info, int accumulate, void *stream);
/* Host pointers, synchronous, built on the _dev form (historystorage.go:50-51, naive.go:199-213, 235-257): the
 * scripts are given; upload + launch + download. The device buffers are taken for the call from the context's
 * pool. partner may be NULL. */
int nmz_move_profile(nmz_ctx *ctx, const uint64_t *off, const uint64_t *sym, uint32_t n_traces, const uint32_t *pairs,
                     uint64_t n_pairs, uint32_t band, const uint32_t *dist, const nmz_edit_op *ops,
                     const uint64_t *usym, uint64_t n_usym, uint32_t *partner /* may be NULL */,
                     nmz_move_counts *counts, nmz_move_info *info);
/* From the traces to the profile (historystorage.go:50-51, naive.go:199-213, 235-257): the CSR goes up, the pairs
 * are aligned (k_ed_align) and profiled on the device; only dist (may be NULL), counts and info come back, the ops
 * never leave the device. Plan and buffers are taken for the call from the context's pool, as nmz_ed_align_pairs
 * takes them. The result is byte-identical to nmz_move_profile over nmz_ed_align_pairs' output. */
int nmz_ed_diff_profile(nmz_ctx *ctx, const uint64_t *off, const uint64_t *sym, uint32_t n_traces,
                        const uint32_t *pairs, uint64_t n_pairs, uint32_t band, const uint64_t *usym, uint64_t n_usym,
                        uint32_t *dist /* may be NULL */, nmz_move_counts *counts, nmz_move_info *info);

/* ---- move profiles over wider bands: 0 <= band <= NMZ_ALIGN_WIDE_MAX_BAND ----------------------------------------
 * The same build-defined extension (historystorage/historystorage.go:50-51; naive/naive.go:235-257; the labels
 * naive.go:199-213), with the semantics above word for word over the scripts nmz_ed_align_wide_* gives: names,
 * partners, direction, span, nmz_move_counts, nmz_move_info, n_unknown, n_beyond for dist > band or dist ==
 * NMZ_NONE, partner[n_pairs * band] with NMZ_NONE wherever a slot has no partner. Every band 0 .. 1024 is accepted:
 * for band <= NMZ_ALIGN_MAX_BAND these entry points return byte for byte what their narrow counterparts return (they
 * run the same kernel), beyond it k_script_moves_wide does the work. Limits of the host-pointer forms, each
 * NMZ_EINVAL with a message, checked before any device work (arguments before the context): band <=
 * NMZ_ALIGN_WIDE_MAX_BAND; n_pairs * band < 2^32 (at band 1024 just under 4 Mi pairs); everything
 * nmz_ed_align_wide_pairs checks, with its messages; usym strictly increasing; where ops are an input, for the first
 * dist slots of every script: kind <= 2, a_pos < n for DEL / SUB, b_pos < m for INS / SUB (the message names pair and
 * slot). n_pairs == 0 is legal and needs no device: the counters and the info are zero. nmz_script_moves_host takes a
 * script of any length as it is. */
/* The whole profile on the calling host thread, plain loops, no device work (historystorage.go:50-51,
 * naive.go:199-213, 235-257): nmz_move_profile_host's body behind the wider band limit, for callers without a device,
 * and the check of the device forms (it shares nothing with the kernels). dist[n_pairs] and ops[n_pairs * band] as
 * nmz_ed_align_wide_pairs writes them; partner[n_pairs * band] may be NULL. */
int nmz_move_profile_wide_host(const uint64_t *off, const uint64_t *sym, uint32_t n_traces, const uint32_t *pairs,
                               uint64_t n_pairs, uint32_t band, const uint32_t *dist, const nmz_edit_op *ops,
                               const uint64_t *usym, uint64_t n_usym, uint32_t *partner /* may be NULL */,
                               nmz_move_counts *counts /* [n_usym] */, nmz_move_info *info);
/* Device pointers in and out (historystorage.go:50-51, naive.go:199-213, 235-257); enqueued on `stream` (NULL = the
 * context's). accumulate as for nmz_move_profile_dev: 0 clears d_counts[n_usym] and d_info on that stream first,
 * otherwise the call adds to them. Apart from the clear it enqueues one launch and allocates nothing. The host
 * cannot read the inputs: n_pairs * band < 2^32 and d_usym strictly increasing are the caller's to keep, offsets and
 * pairs as for nmz_ed_align_wide_pairs_dev; an op of a script with kind > 2 or a position outside its trace counts
 * for nothing (no name, no partner), and the kernel makes no out-of-range read for it. d_partner[n_pairs * band] may
 * be NULL. */
int nmz_move_profile_wide_dev(nmz_ctx *ctx, const uint64_t *d_off, const uint64_t *d_sym, const uint32_t *d_pairs,
                              uint64_t n_pairs, uint32_t band, const uint32_t *d_dist, const nmz_edit_op *d_ops,
                              const uint64_t *d_usym, uint64_t n_usym, uint32_t *d_partner /* may be NULL */,
                              nmz_move_counts *d_counts, nmz_move_info *d_info, int accumulate, void *stream);
/* Host pointers, synchronous, built on the _dev form (historystorage.go:50-51, naive.go:199-213, 235-257): the
 * scripts are given; upload + launch + download. The device buffers are taken for the call from the context's
 * pool. partner may be NULL. */
int nmz_move_profile_wide(nmz_ctx *ctx, const uint64_t *off, const uint64_t *sym, uint32_t n_traces,
                          const uint32_t *pairs, uint64_t n_pairs, uint32_t band, const uint32_t *dist,
                          const nmz_edit_op *ops, const uint64_t *usym, uint64_t n_usym,
                          uint32_t *partner /* may be NULL */, nmz_move_counts *counts, nmz_move_info *info);
/* From the traces to the profile (historystorage.go:50-51, naive.go:199-213, 235-257): the CSR goes up, the pairs
 * are aligned (k_ed_align_wide on a plan taken for the call from the context's pool) and profiled on the device;
 * only dist (may be NULL), counts and info come back, the ops never leave the device. The result is byte-identical
 * to nmz_move_profile_wide over nmz_ed_align_wide_pairs' output. */
int nmz_ed_diff_profile_wide(nmz_ctx *ctx, const uint64_t *off, const uint64_t *sym, uint32_t n_traces,
                             const uint32_t *pairs, uint64_t n_pairs, uint32_t band, const uint64_t *usym,
                             uint64_t n_usym, uint32_t *dist /* may be NULL */, nmz_move_counts *counts,
                             nmz_move_info *info);

/* ---- edit scripts and move profiles per entity: the partial-order view of a diff -----------------------------
 * The same build-defined extension (historystorage/historystorage.go:50-51; the reference has equality only,
 * naive/naive.go:235-257) in the reference's partial-order mode (cli/tools/visualize.go:62-136, createTracesPerEntity
 * and tracesEqualInPO; `visualize`'s po_reduction defaults to true). Inputs: the CSR off / sym and entity[N] (uint32),
 * parallel to sym: ids global to the store (equal ids in two traces mean the same entity -- unlike nmz_unique_traces,
 * whose ids are dense per trace), each < n_entities or NMZ_NONE for an action without an event (skipped, as
 * nmz_unique_traces skips it); 1 <= n_entities <= NMZ_PO_MAX_ENTITIES; a band 0 .. NMZ_ALIGN_WIDE_MAX_BAND.
 *   Projection. t|g is the subsequence of trace t's elements with entity g, in order; src_g(t)[p] the index in t of
 *               its p-th element; lift_g(t, p) = src_g(t)[p] for p < |t|g|, and |t| for p = |t|g|.
 *   Distance.   dist = min(sum over g of Lev(a|g, b|g), band + 1): exact (one Lev_g > band puts the sum beyond it).
 *               dist == 0 <=> the entity sets and every per-entity sequence are equal <=> tracesEqualInPO.
 *   Script.     For dist <= band exactly dist ops: for g = 0, 1, ... in ascending id the canonical script of
 *               (a|g, b|g) as defined above, every a_pos replaced by lift_g(a, a_pos) and every b_pos by
 *               lift_g(b, b_pos), concatenated in entity order; sentinels in the remaining slots. The entity of an op
 *               is entity_a[a_pos] for DEL / SUB and entity_b[b_pos] for INS. Within one entity's segment the slots
 *               keep script order; positions are not monotone across segments.
 * The lifted ops satisfy what nmz_move_profile_wide* validates, and those kernels assume no position order: the move
 * profile of a PO script is what nmz_move_profile_wide_host returns for it over the original CSR. With n_entities == 1
 * and no NMZ_NONE the entry points return byte for byte what nmz_ed_align_wide_* return. Limits, each NMZ_EINVAL with
 * a message, checked before any device work (arguments before the context): everything nmz_ed_align_wide_pairs
 * checks, with its messages; entity non-NULL when there is any element; 1 <= n_entities <= NMZ_PO_MAX_ENTITIES; every
 * id < n_entities or NMZ_NONE (the message names the element); n_traces * n_entities < 2^31 - 1 (the projected traces
 * are indexed with 32 bits). n_pairs == 0 needs no device; band == 0 is legal with ops NULL. */
#define NMZ_PO_MAX_ENTITIES 1024
/* Device pointers in and out (historystorage.go:50-51, naive.go:235-257, visualize.go:62-136): the stable partition
 * of every trace by entity, enqueued on `stream` (NULL = the context's): a count pass, one scan, a scatter pass.
 * d_poff[n_traces * n_entities + 1] (uint64): projected trace t * n_entities + g is d_psym[d_poff[.] .. d_poff[. +
 * 1]), an ordinary CSR; d_psrc[q] (uint32) is the index in its trace of the element at d_psym[q]. d_psym and d_psrc
 * hold as many elements as d_sym. The host cannot read the ids: NMZ_NONE and, here, ids >= n_entities are dropped and
 * never indexed with. The scan's temporary is a scratch slot of the context. */
int nmz_po_project_dev(nmz_ctx *ctx, const uint64_t *d_off, const uint64_t *d_sym, const uint32_t *d_entity,
                       uint32_t n_traces, uint32_t n_entities, uint64_t *d_poff, uint64_t *d_psym, uint32_t *d_psrc,
                       void *stream);
/* Host pointers, synchronous, built on the _dev form (historystorage.go:50-51, naive.go:235-257,
 * visualize.go:62-136): upload + project + download. poff[n_traces * n_entities + 1]; psym and psrc receive
 * poff[n_traces * n_entities] elements (the elements whose id is not NMZ_NONE). */
int nmz_po_project(nmz_ctx *ctx, const uint64_t *off, const uint64_t *sym, const uint32_t *entity, uint32_t n_traces,
                   uint32_t n_entities, uint64_t *poff, uint64_t *psym, uint32_t *psrc);
/* One pair on the calling host thread, no device work (historystorage.go:50-51, naive.go:235-257,
 * visualize.go:62-136): plain vectors per entity, nmz_ed_align_wide_host's DP per entity, lift, concatenate. It shares
 * nothing with the kernels: the check of the device forms. ea[n] / eb[m] are the entities of a / b. */
int nmz_ed_align_po_host(const uint64_t *a, const uint32_t *ea, uint64_t n, const uint64_t *b, const uint32_t *eb,
                         uint64_t m, uint32_t n_entities, uint32_t band, uint32_t *dist,
                         nmz_edit_op *ops /* [band] */);
/* The plan owns a wide align plan for projections of up to max_len elements and the sub-pair scratch for max_pairs
 * pairs per launch (historystorage.go:50-51, naive.go:235-257, visualize.go:62-136): per pair and entity one pair of
 * projected traces, its distance and `band` op slots. The plan serves one stream at a time (a launch on another
 * stream waits for the one before); destroy waits for its launches. */
typedef struct nmz_ed_align_po_plan nmz_ed_align_po_plan;
int nmz_ed_align_po_plan_create(nmz_ctx *ctx, uint32_t band, uint32_t n_entities, uint64_t max_len,
                                uint64_t max_pairs, nmz_ed_align_po_plan **out);
int nmz_ed_align_po_plan_destroy(nmz_ed_align_po_plan *plan);
/* The plan's constants (historystorage.go:50-51, naive.go:235-257, visualize.go:62-136): the inner plan's pairs in
 * flight and history bytes, and the bytes of sub-pair scratch; each pointer may be NULL. */
int nmz_ed_align_po_plan_info(const nmz_ed_align_po_plan *plan, uint32_t *slots, uint64_t *history_bytes,
                              uint64_t *sub_pair_bytes);
/* The original offsets, nmz_po_project_dev's outputs and device pairs in, d_dist[n_pairs] and d_ops[n_pairs * band]
 * out (historystorage.go:50-51, naive.go:235-257, visualize.go:62-136); enqueued on `stream` (NULL = the context's):
 * the sub-pairs, the aligner over them and the gather, nothing else. n_pairs > max_pairs is NMZ_EINVAL. A pair with a
 * projection longer than the plan's max_len gets dist = NMZ_NONE and sentinel ops. */
int nmz_ed_align_po_pairs_dev(nmz_ed_align_po_plan *plan, const uint64_t *d_off, const uint64_t *d_poff,
                              const uint64_t *d_psym, const uint32_t *d_psrc, const uint32_t *d_pairs,
                              uint64_t n_pairs, uint32_t *d_dist, nmz_edit_op *d_ops /* [n_pairs * band] */,
                              void *stream);
/* Host pointers, synchronous, built on the _dev forms (historystorage.go:50-51, naive.go:235-257,
 * visualize.go:62-136): upload + project + a plan for the longest projection among the pairs' traces + launches +
 * download. The sub-pair scratch is capped at 256 MiB, so the pairs run in batches of max(1, 256 MiB / (n_entities *
 * band * 12)) on one stream; the results do not depend on the batch size. */
int nmz_ed_align_po_pairs(nmz_ctx *ctx, const uint64_t *off, const uint64_t *sym, const uint32_t *entity,
                          uint32_t n_traces, uint32_t n_entities, const uint32_t *pairs, uint64_t n_pairs,
                          uint32_t band, uint32_t *dist, nmz_edit_op *ops);
/* From the traces to the PO profile (historystorage.go:50-51, naive.go:199-213, 235-257, visualize.go:62-136):
 * project, the PO scripts, then k_script_moves_wide accumulating over the batches; the ops never leave the device.
 * The result is byte-identical to nmz_move_profile_wide over nmz_ed_align_po_pairs' output. */
int nmz_ed_diff_profile_po(nmz_ctx *ctx, const uint64_t *off, const uint64_t *sym, const uint32_t *entity,
                           uint32_t n_traces, uint32_t n_entities, const uint32_t *pairs, uint64_t n_pairs,
                           uint32_t band, const uint64_t *usym, uint64_t n_usym, uint32_t *dist /* may be NULL */,
                           nmz_move_counts *counts, nmz_move_info *info);

/* ---- PO k-NN search: the k nearest stored runs by per-entity edit distance ---------------------------------------
 * The same build-defined extension (historystorage/historystorage.go:50-51; naive/naive.go:235-257;
 * cli/tools/visualize.go:62-136): the search that goes with the per-entity scripts above. The store is a CSR off / sym
 * with entity[N] exactly as nmz_ed_align_po_pairs takes them; the queries are a second CSR q_off / q_sym / q_entity
 * over the same id space; q_self[Q] (uint32, optional) is the store index a query must skip, NMZ_NONE for none, NULL
 * for none at all (queries = the store and q_self[i] = i: an all-pairs k-NN).
 *   d(q, c) = ED^PO_band(query q, stored c) = min(sum over g of Lev(q|g, c|g), band + 1); d == 0 <=> tracesEqualInPO.
 *   Result.   Per query the k smallest keys d << 32 | c over the stored c != q_self[q], ascending: (distance asc, id
 *             asc), nmz_ed_plan_query_knn's order. Pairs beyond the band are listed at d = band + 1, smallest ids
 *             first. Slots past the number of eligible stored traces hold NMZ_NONE / NMZ_NONE (UINT64_MAX as a key).
 *             With n_entities == 1 and no NMZ_NONE the lists equal nmz_ed_plan_query_knn's over the same store.
 *   Filter.   Every trace has a 256-byte profile of its projection: lenfold[b] (b < 32, uint32) = the sum of |t|g|
 *             over g = b (mod 32), and gram[h] (h < 128, uint8 saturating at 255) = the number of positions p of any
 *             t|g with mix(mix(prev + g) ^ cur) >> 57 == h, cur = t|g[p], prev = t|g[p - 1] or 0x9E3779B97F4A7C15 at
 *             p == 0, mix the splitmix64 finaliser. LB_len = sum_b |lenfold_q[b] - lenfold_c[b]| and LB_gram =
 *             ceil(sum_h |gram_q[h] - gram_c[h]| / 4) are lower bounds of sum_g Lev_g, so max(LB_len, LB_gram) > band
 *             settles d = band + 1 exactly: the filter never changes a result.
 * Limits, each NMZ_EINVAL with a message, checked before any device work (arguments before the context):
 * band <= NMZ_PO_KNN_MAX_BAND; 1 <= k <= NMZ_PO_KNN_MAX_K; 1 <= n_entities <= NMZ_PO_MAX_ENTITIES; offsets starting at
 * 0 and non-decreasing; traces shorter than 2^32 - 1; every id < n_entities or NMZ_NONE (the message names the element
 * and whether it is a store or a query element); n_traces * n_entities < 2^31 - 1 and the same for the queries;
 * q_self[i] < n_traces or NMZ_NONE. n_queries == 0 needs no device; n_traces == 0 gives all NMZ_NONE; band == 0 is the
 * search for PO-equal runs. */
#define NMZ_PO_KNN_MAX_BAND 64
#define NMZ_PO_KNN_MAX_K 64
#define NMZ_PO_KNN_OPT_NO_FILTER 1u /* every pair takes the DP path (A/B and tests); the lists do not change */
#define NMZ_PO_KNN_OPT_WHOLE_BLOCKS 2u /* a block's survivors stay with one wave (A/B and tests); the same lists */
#define NMZ_PO_KNN_NCOUNTERS 4
/* Uploads the store, projects it, profiles it and keeps the projection and the profiles resident; sizes the
 * query-side scratch of the _dev form for max_queries queries of max_query_elems elements in all
 * (historystorage.go:50-51, naive.go:235-257, visualize.go:62-136). Synchronous. The plan serves one stream at a time
 * (a launch on another stream waits for the one before); destroy waits for its launches. */
typedef struct nmz_po_knn_plan nmz_po_knn_plan;
int nmz_po_knn_plan_create(nmz_ctx *ctx, const uint64_t *off, const uint64_t *sym, const uint32_t *entity,
                           uint32_t n_traces, uint32_t n_entities, uint32_t band, uint64_t max_queries,
                           uint64_t max_query_elems, uint32_t opts, nmz_po_knn_plan **out);
int nmz_po_knn_plan_destroy(nmz_po_knn_plan *plan);
/* The plan's resident bytes (projected store, profiles, query scratch) and the workgroups and waves of its latest
 * search kernel launch (historystorage.go:50-51, naive.go:235-257, visualize.go:62-136); each pointer may be NULL. */
int nmz_po_knn_plan_info(const nmz_po_knn_plan *plan, uint64_t *resident_bytes, uint32_t *blocks, uint32_t *waves);
/* Device pointers in, d_knn_keys[n_queries * k] (uint64 keys) out (historystorage.go:50-51, naive.go:235-257,
 * visualize.go:62-136); enqueued on `stream` (NULL = the context's) and nothing else: the queries' projection and
 * profiles, the search, the fill. n_queries > max_queries is NMZ_EINVAL (the message names both). The host cannot read
 * d_q_off: offsets that do not start at 0, decrease or pass max_query_elems never leave the plan's scratch, the search
 * then writes no list (every key stays UINT64_MAX) and nmz_po_knn_counters reports it. Query ids >= n_entities are
 * dropped like NMZ_NONE; d_q_self may be NULL. n_queries == 0 enqueues nothing. */
int nmz_po_knn_query_dev(nmz_po_knn_plan *plan, const uint64_t *d_q_off, const uint64_t *d_q_sym,
                         const uint32_t *d_q_entity, const uint32_t *d_q_self, uint32_t n_queries, uint32_t k,
                         uint64_t *d_knn_keys, void *stream);
/* Host pointers, synchronous, every limit checked (historystorage.go:50-51, naive.go:235-257, visualize.go:62-136):
 * the queries run in batches of at most max_queries queries and max_query_elems elements on the context's stream; one
 * query longer than max_query_elems is NMZ_EINVAL (the message names both). knn_id / knn_dist [n_queries * k]. */
int nmz_po_knn_query(nmz_po_knn_plan *plan, const uint64_t *q_off, const uint64_t *q_sym, const uint32_t *q_entity,
                     const uint32_t *q_self /* may be NULL */, uint32_t n_queries, uint32_t k, uint32_t *knn_id,
                     uint32_t *knn_dist);
/* One shot (historystorage.go:50-51, naive.go:235-257, visualize.go:62-136): a plan for this store and these queries,
 * the search, the plan's release; the buffers come from the context's pool. */
int nmz_po_knn(nmz_ctx *ctx, const uint64_t *off, const uint64_t *sym, const uint32_t *entity, uint32_t n_traces,
               uint32_t n_entities, const uint64_t *q_off, const uint64_t *q_sym, const uint32_t *q_entity,
               const uint32_t *q_self /* may be NULL */, uint32_t n_queries, uint32_t band, uint32_t k,
               uint32_t *knn_id, uint32_t *knn_dist);
/* The latest search's work (historystorage.go:50-51, naive.go:235-257, visualize.go:62-136), read after `stream`
 * (NULL = the context's) has drained: out[0] pairs settled by the filter, out[1] pairs settled by the exact sum of the
 * entities' length differences, out[2] pairs that ran a DP, out[3] pairs in band. Eligible pairs = out[0] + out[1] +
 * out[2]. */
int nmz_po_knn_counters(nmz_po_knn_plan *plan, uint64_t *out /* [NMZ_PO_KNN_NCOUNTERS] */, void *stream);
/* The two lower bounds of one pair on the calling host thread, by the definition above, no device work
 * (historystorage.go:50-51, naive.go:235-257, visualize.go:62-136). It shares no table with the kernels: the check of
 * the filter. */
int nmz_po_knn_bound_host(const uint64_t *a, const uint32_t *ea, uint64_t n, const uint64_t *b, const uint32_t *eb,
                          uint64_t m, uint32_t n_entities, uint32_t *lb_len, uint32_t *lb_gram);

/* ---- PO k-NN search over bands up to 1,024 ---------------------------------------------------------------------------
 * The search above, word for word, with 0 <= band <= NMZ_PO_KNN_WIDE_MAX_BAND (historystorage/historystorage.go:50-51;
 * naive/naive.go:235-257; cli/tools/visualize.go:62-136): the neighbours that go with nmz_ed_align_po_pairs' scripts
 * at the bands real stores need. The plan type is the narrow form's, and nmz_po_knn_plan_destroy, _plan_info,
 * _query_dev, _query and _counters serve a plan of either create. A band above 64 searches with k_po_knn_wide (four
 * waves per pair; every entity's band clamped to min(what is left of the band, the longer projection), which is
 * exact since Lev <= max(n, m)); a band <= 64 runs the narrow kernel and gives the narrow entry points' bytes and
 * counters. The profiles, the two lower bounds and nmz_po_knn_bound_host do not depend on the band.
 * Limits: band > NMZ_PO_KNN_WIDE_MAX_BAND is NMZ_EINVAL; every other limit, message and order of checks is the narrow
 * form's. The narrow entry points keep NMZ_PO_KNN_MAX_BAND. */
#define NMZ_PO_KNN_WIDE_MAX_BAND 1024
#define NMZ_PO_KNN_WIDE_NCOUNTERS 9
/* nmz_po_knn_wide_plan_create only: every entity laid out for the plan's band, not for its clamped one (A/B and
 * tests); the lists do not change. Without effect at a band <= 64. */
#define NMZ_PO_KNN_OPT_FULL_BAND 4u
/* nmz_po_knn_plan_create for every band 0 .. 1,024 (historystorage.go:50-51, naive.go:235-257,
 * visualize.go:62-136). */
int nmz_po_knn_wide_plan_create(nmz_ctx *ctx, const uint64_t *off, const uint64_t *sym, const uint32_t *entity,
                                uint32_t n_traces, uint32_t n_entities, uint32_t band, uint64_t max_queries,
                                uint64_t max_query_elems, uint32_t opts, nmz_po_knn_plan **out);
/* nmz_po_knn for every band 0 .. 1,024, one shot (historystorage.go:50-51, naive.go:235-257,
 * visualize.go:62-136). */
int nmz_po_knn_wide(nmz_ctx *ctx, const uint64_t *off, const uint64_t *sym, const uint32_t *entity, uint32_t n_traces,
                    uint32_t n_entities, const uint64_t *q_off, const uint64_t *q_sym, const uint32_t *q_entity,
                    const uint32_t *q_self /* may be NULL */, uint32_t n_queries, uint32_t band, uint32_t k,
                    uint32_t *knn_id, uint32_t *knn_dist);
/* nmz_po_knn_counters' four words, then out[4 .. 8]: the entity steps (one banded DP of one entity of one pair) that
 * the latest search ran at 1, 2, 3, 5 and 9 cells per thread, i.e. at a clamped band <= 127, 255, 383, 639 and 1,024
 * (historystorage.go:50-51, naive.go:235-257, visualize.go:62-136). All 0 for a plan whose band is <= 64. */
int nmz_po_knn_wide_counters(nmz_po_knn_plan *plan, uint64_t *out /* [NMZ_PO_KNN_WIDE_NCOUNTERS] */, void *stream);

/* ---- device groups: several GPUs behind one call (multi-GPU inside the C ABI) ----------------------------
 * The reference's callers are single processes (cli/run.go:123-136 initPolicy; cli/tools/visualize.go:138-172),
 * so one process must reach every GPU of a node. A group holds one context and one worker thread per device
 * (bound to its device once, so a cgo caller may call from any OS thread) and one RCCL communicator over the
 * devices, created once. Work is cut into n_shards shards (0 = one per rank; more than the ranks = "virtual"
 * shards, so a single GPU runs the sharding and merge logic of any shard count); shard s runs on rank
 * s mod n_ranks. Sweeps shard by contiguous seed range (sizes differ by <= 1), the all-pairs search by the
 * plan's query-block deal (rotated snake order, nmz_ed_block_shard). Each rank merges its shards on its device,
 * one RCCL
 * all_gather over xGMI exchanges the ranks' lists, and a deterministic merge -- (n_fault desc, sum_delay desc,
 * seed asc) for top-k, (dist asc, id asc) for k-NN -- makes the result identical to one unsharded call.
 * Group calls are synchronous and serialised per group; host buffers are borrowed for the call only. A group call
 * never changes the calling thread's current HIP device (nor does any single-context call). */
typedef struct nmz_group nmz_group;
#define NMZ_GROUP_ID_BYTES 128
/* bit d of dev_mask = device d */
int nmz_open_group(uint32_t dev_mask, uint32_t n_shards, nmz_group **out);
/* One process per device (several hosts, or a launcher with a process per GPU): rank 0 makes the id
 * (nmz_group_unique_id) and hands it to every rank out of band; each rank opens its device. Every rank receives
 * the merged results. stats outputs hold the seeds of this rank's shards only. */
int nmz_group_unique_id(uint8_t *id /* [NMZ_GROUP_ID_BYTES] */);
int nmz_open_group_rank(const uint8_t *id, int n_ranks, int rank, int device, uint32_t n_shards, nmz_group **out);
/* Waits for a group call already in progress, then frees the group; NMZ_EINVAL while group plans made on it are
 * still alive (destroy them first). No call on the group may start once close has begun. */
int nmz_close_group(nmz_group *g);
int nmz_group_info(const nmz_group *g, int *n_ranks, int *n_local_devices, uint32_t *n_shards);
/* Collectives this process has entered on the group so far. Every group call that exchanges results first enters
 * one status all_gather (every rank, whatever failed locally) and then, only when every rank succeeded, its payload
 * collective, so a failed call enters the same collectives on every rank (tests check the sequence with this). */
int nmz_group_collectives(const nmz_group *g, uint64_t *n);

/* replayable sweep over a group (replayablepolicy.go:100-114 per decision, as nmz_replayable_sweep): one plan
 * per device, kept for repeated sweeps; stats[n_seeds] (may be NULL) and the merged topk[k] (k <= 256, .seed =
 * seed index, or the seed's integer value for the decimal form) go to host memory. */
typedef struct nmz_replayable_group_plan nmz_replayable_group_plan;
int nmz_replayable_group_plan_create(nmz_group *g, const uint32_t *hint_off, const uint8_t *hint_bytes,
                                     uint32_t n_events, int64_t max_interval_ns, uint64_t max_seeds_per_shard,
                                     nmz_replayable_group_plan **out);
int nmz_replayable_group_plan_destroy(nmz_replayable_group_plan *gp);
int nmz_replayable_group_sweep(nmz_replayable_group_plan *gp, const uint32_t *seed_off, const uint8_t *seed_bytes,
                               uint64_t n_seeds, uint32_t k, nmz_sched_stats *stats, nmz_topk_entry *topk);
/* seeds = decimal strings of seed_lo .. seed_lo + n_seeds - 1 (nmz_replayable_sweep_decimal_topk_dev) */
int nmz_replayable_group_sweep_decimal(nmz_replayable_group_plan *gp, uint64_t seed_lo, uint64_t n_seeds, uint32_t k,
                                       nmz_sched_stats *stats, nmz_topk_entry *topk);
/* one call: plan + sweep + merged top-k (the group form of nmz_replayable_sweep) */
int nmz_replayable_sweep_topk_group(nmz_group *g, const uint32_t *seed_off, const uint8_t *seed_bytes,
                                    uint64_t n_seeds, const uint32_t *hint_off, const uint8_t *hint_bytes,
                                    uint32_t n_events, int64_t max_interval_ns, uint32_t k, nmz_sched_stats *stats,
                                    nmz_topk_entry *topk);

/* random-policy sweep over a group (randompolicy.go:300-346, as nmz_random_sweep): seeds seed0 .. seed0+n-1. */
typedef struct nmz_random_group_plan nmz_random_group_plan;
int nmz_random_group_plan_create(nmz_group *g, const uint64_t *evhash, const uint8_t *evclass, uint32_t n_events,
                                 const nmz_random_params *params, uint64_t max_seeds_per_shard,
                                 nmz_random_group_plan **out);
int nmz_random_group_plan_destroy(nmz_random_group_plan *gp);
int nmz_random_group_sweep(nmz_random_group_plan *gp, uint64_t seed0, uint64_t n_seeds, uint32_t k,
                           nmz_sched_stats *stats, nmz_topk_entry *topk);
int nmz_random_sweep_topk_group(nmz_group *g, uint64_t seed0, uint64_t n_seeds, const uint64_t *evhash,
                                const uint8_t *evclass, uint32_t n_events, const nmz_random_params *params,
                                uint32_t k, nmz_sched_stats *stats, nmz_topk_entry *topk);

/* all-pairs banded edit-distance k-NN over a group (as nmz_ed_allpairs_knn): every device holds the store. The
 * store reaches the devices as 1/n_ranks shares: rank r uploads symbols [r S, r S + S) (S = ceil(total / n_ranks))
 * through its own PCIe link, one RCCL all_gather over xGMI assembles the store on every device, and each device
 * builds its plan from device memory (nmz_ed_plan_create_dev). nmz_ed_group_plan_timing reports, per local device,
 * the share upload, the all_gather and the device plan build (ms, arrays of nmz_group_info's n_local_devices).
 * After each local step (upload, plan build) the ranks exchange their status, so a rank that failed never leaves the
 * others waiting in a collective; after the build they exchange their plans' fingerprints (nmz_ed_plan_fingerprint)
 * and all fail with NMZ_EINVAL when any two differ. */
typedef struct nmz_ed_group_plan nmz_ed_group_plan;
int nmz_ed_group_plan_create(nmz_group *g, const uint64_t *off, const uint64_t *sym, uint32_t n_traces,
                             uint32_t band, nmz_ed_group_plan **out);
/* The same with NMZ_ED_OPT_* plan options for every member's plan (nmz_ed_plan_create_opts). */
int nmz_ed_group_plan_create_opts(nmz_group *g, const uint64_t *off, const uint64_t *sym, uint32_t n_traces,
                                  uint32_t band, uint32_t opts, nmz_ed_group_plan **out);
int nmz_ed_group_plan_timing(const nmz_ed_group_plan *gp, double *upload_ms, double *gather_ms, double *build_ms);
int nmz_ed_group_plan_destroy(nmz_ed_group_plan *gp);
int nmz_ed_group_allpairs_knn(nmz_ed_group_plan *gp, uint32_t k, uint32_t *knn_id, uint32_t *knn_dist);
int nmz_ed_allpairs_knn_group(nmz_group *g, const uint64_t *off, const uint64_t *sym, uint32_t n_traces,
                              uint32_t band, uint32_t k, uint32_t *knn_id, uint32_t *knn_dist);

#ifdef __cplusplus
}
#endif
#endif /* NMZ_GPU_H */
