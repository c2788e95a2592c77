// K1 (replayable sweep) declarations shared by its translation units: the plan and the prepared seed set, and the
// entry points of each kernel family -- seed prefixes (replayable_seeds.hip), per-decision sweeps
// (replayable_pd.hip), order-query statistics (replayable_oq.hip), wavelet-tree statistics (replayable_wt_plan.hip, replayable_wt.hip).
// replayable.hip holds the plan's build, the dispatch and the C ABI.
#pragma once
#include <array>

#include "nmz_common.h"
#include "nmz_internal.h"

namespace nmz {

// replayable plan: one hint-length class (a segment of every table row)
struct ClassInfo {
    uint64_t pn;     // P^len
    uint32_t start;  // first position in the length-sorted event order
    uint32_t count;
};

// ---- seed prefixes and seed scratch (replayable_seeds.hip) ----
// smallest per-decision work unit (64 lanes x REPLAY_U = 2 seeds): sizes the unit list of every seed scratch
constexpr uint32_t REPLAY_SEEDS_PER_UNIT_MIN = 64 * 2;
// seeds per workgroup of the statistics kernels (16 waves share one staged row): their bucketing granularity
constexpr uint32_t OQ_WG = 1024;

struct SeedScratch {
    uint64_t *h0;
    Buckets b;
    uint32_t *small;  // b's offset, n_units and total (buckets_small)
    uint32_t *counter;
};

// the fields of a seed scratch for S seeds, appended to lay; seed_scratch_bind sizes a buffer for them,
// carve_seed_scratch finds them again in a buffer that seed_scratch_bind sized for the same S
inline void seed_scratch_layout(ScratchLayout &lay, uint64_t S, SeedScratch &s) {
    lay.add(&s.h0, S).add(&s.b.sorted_h0, S).add(&s.b.sorted_idx, S).add(&s.small, BUCKET_SMALL_U32);
    lay.add(&s.b.hist, bucket_hist_u32(S)).add(&s.b.units, S / REPLAY_SEEDS_PER_UNIT_MIN + 257).add(&s.counter, 4);
}

inline int seed_scratch_bind(DevBuf &buf, uint64_t S, SeedScratch &s) {
    ScratchLayout lay;
    seed_scratch_layout(lay, S, s);
    NMZ_TRY(lay.bind(buf));
    buckets_small(s.small, s.b);
    return NMZ_OK;
}

inline SeedScratch carve_seed_scratch(void *p, uint64_t S) {
    ScratchLayout lay;
    SeedScratch s;
    seed_scratch_layout(lay, S, s);
    (void)lay.place(p);
    buckets_small(s.small, s.b);
    return s;
}

// the seeds' prefix hashes (also for order.hip): h0[S] = FNV-1a 64 of each seed string of the device CSR
// (k_seed_prefix), or (d_soff == nullptr) of the decimal strings of dec_lo .. dec_lo + S - 1, wrapping past 2^64
// (k_seed_prefix_decimal); rows[bucket_hist_u32(S)] receives the kernels' bucket counts
int seed_prefix_launch(hipStream_t st, const uint32_t *d_soff, const uint8_t *d_sbytes, uint64_t dec_lo, uint64_t S,
                       uint64_t *h0, uint32_t *rows);
// the caller holds ctx (nmz_replayable_seeds_create, nmz_replayable_sweep_traces)
int seeds_create_locked(nmz_ctx *ctx, const uint32_t *d_seed_off, const uint8_t *d_seed_bytes, uint64_t n_seeds,
                        uint64_t dec_lo, nmz_replayable_seeds **out);
void seeds_destroy_locked(nmz_replayable_seeds *seeds);

// ---- order-query statistics (replayable_oq.hip): per-row blobs staged whole into LDS, one blob per pass (a row
// whose image exceeds LDS is split into passes over disjoint class segments; the per-seed statistics of the passes
// combine: sums add, maxima max) ----
struct OqClass;
struct OqState {
    bool on = false;
    struct Pass {
        uint32_t c0, c1;  // OqClass range of the pass
        uint64_t off16;   // first uint4 of the pass's [256][rb16] images in d_blob
        uint32_t rb16;    // row image bytes / 16
    };
    std::vector<Pass> passes;
    uint4 *d_blob = nullptr;       // per pass [256][rb16] row images (level arrays {Cm, ~e} + samples of C)
    uint64_t *d_rowsum = nullptr;  // [passes][256] sum of C mod m over the pass's part of the row
    OqClass *d_classes = nullptr;
    DevBuf mem;
};
// order-query statistics (default) or the per-decision sweep (NMZ_REPLAY_OQ=0, for tests and A/B runs)
bool replay_oq_enabled();
// builds the row images after the C sort when they apply (0 < m < 2^32; o.on says whether they do)
int oq_build(OqState &o, const uint4 *d_table, uint32_t E, const ModParams &mod, const std::vector<ClassInfo> &cls,
             hipStream_t st);
// one kernel run per pass over seeds bucketed at OQ_WG
int oq_sweep(const OqState &o, nmz_ctx *ctx, hipStream_t st, const Buckets &b, const uint4 *d_table, uint32_t E,
             const ModParams &mod, nmz_sched_stats *d_stats);

// ---- K1 wavelet-tree statistics: per-row images built once per plan (replayable_wt_plan.hip), staged into LDS per
// sweep (replayable_wt.hip, with the top-k selection of replayable_wt_topk_dev.h) ----
struct WtState {
    bool on = false;
    uint32_t rb16 = 0, n_classes = 0, msh = 0;
    uint32_t bb = 5;                        // rank blocks of 2^bb ranks below the tree's levels (replayable_wt_dev.h)
    bool planes = false;                    // rank-block planes instead of levels (bb = 6, every segment or none)
    uint4 *d_blob = nullptr;                // [256][rb16] row images
    unsigned long long *d_rowsum = nullptr;  // [256] sum of C mod m over the row
    void *d_classes = nullptr;              // [n_classes] segment descriptors
    DevBuf mem;                             // the row images
    DevBuf aux;                             // separate path: row sums and segment descriptors
};
bool wt_enabled();
struct WtClass {
    uint64_t pn;              // P^len
    uint32_t start, n;        // table segment (C order)
    uint32_t o_lv, o_cm;      // byte offsets in the row image: wavelet levels [K][nw] {bits, ones before};
    uint32_t o_chi, o_e;      //   Cm by rank (+ sentinel); C's high word by position (+ sentinel); e by rank (u16)
    uint32_t o_im, o_ic;      //   bucket indexes (u16): first rank with Cm >= b << msh (257); first position
                              //   with C_hi >= b << 24 (256)
    uint32_t K, nw;           // rank bits (2^K > n); words per level (n / 32 + 1)
    uint32_t rS;              // lifting-search rounds (the largest bucket's bit length; set by the plan kernel)
    uint32_t o_mk;            //   block masks [(n >> bb) + 1][2^bb + 1] of 2^bb bits: the ranks (bit r mod 2^bb)
                              //   among the first o entries of each 2^bb-rank block's node, o = 0..2^bb
    uint32_t order;           // plan kernel: the segment whose rows the order-th group of 256 workgroups builds
    uint32_t o_pl;            //   rank-block planes [(n >> 6) + 2][nw] {bits, ones before} in place of the levels
                              //   (plane b: rank >= 64 b, in position order), or 0: the segment has levels
};
static_assert(sizeof(WtClass) == 64, "WtClass layout");

// The wavelet-tree images: wt_layout (host only) decides whether they apply and lays out the segments (fused: every
// class must be one segment), wt_launch runs the plan kernel with the classes and zeroed row sums already on the
// device -- with hints (fused) the kernel computes the correction table itself (FNV of each hint per row L, C-sorted
// per class) into hints->table and zeroes the two given ranges; wt_build = the separate path (table built first).
struct WtPlanHints {
    const uint32_t *hoff;
    const uint8_t *hbytes;
    const uint32_t *perm;
    uint4 *table;
    uint32_t *zero0;
    uint32_t n_zero0;
    uint32_t *zero1;
    uint32_t n_zero1;
};
bool wt_layout(WtState &w, nmz_ctx *ctx, uint32_t E, const ClassInfo *cls, uint32_t n_cls, const ModParams &mod,
               bool fused, std::vector<WtClass> &oc);
int wt_launch(WtState &w, const uint4 *d_table, uint32_t E, const ModParams &mod, hipStream_t st,
              const WtPlanHints *hints, WtClass *d_cls, unsigned long long *d_rowsum, bool sync);
int wt_build(WtState &w, nmz_ctx *ctx, const uint4 *d_table, uint32_t E, const ClassInfo *cls, uint32_t n_cls,
             const ModParams &mod, hipStream_t st);
// topk_scratch (wt_topk_scratch_bytes(S), or nullptr): the sweep also leaves one record per 64-seed chunk there for
// wt_topk (the chunk's largest sum, its first sorted position and its seed count)
int wt_sweep(const WtState &w, nmz_ctx *ctx, hipStream_t st, const Buckets &b, const uint4 *d_table, uint32_t E,
             const ModParams &mod, nmz_sched_stats *d_stats, uint64_t S, void *topk_scratch);
size_t wt_topk_scratch_bytes(uint64_t S);
// the top-k (k <= 64) of a sweep that ran with topk_scratch: one kernel, from the chunk records, the sweep's bucketing
// (bucket_off [257], sorted_idx [S]) and its stats
int wt_topk(hipStream_t st, void *scratch, const uint32_t *bucket_off, const uint32_t *sorted_idx,
            const nmz_sched_stats *d_stats, uint64_t S, uint64_t seed0, uint32_t k, nmz_topk_entry *d_out);

// ---- per-decision sweeps (replayable_pd.hip): k_replayable_sweep_fast + k_replayable_merge for m < 2^30,
// k_replayable_sweep_general otherwise; buckets the hashes sc.h0 (sc.b.hist holds their row counts) at its own
// granularity ----
int pd_sweep(nmz_replayable_plan *p, hipStream_t st, SeedScratch &sc, uint64_t S, nmz_sched_stats *d_stats);

}  // namespace nmz

struct nmz_replayable_plan {
    nmz_ctx *ctx = nullptr;
    uint32_t n_events = 0;
    int64_t max_interval = 0;
    nmz::ModParams mod{};
    uint32_t n_classes = 0;
    nmz::ClassInfo *d_classes = nullptr;
    uint4 *d_table = nullptr;          // [256][E] {C lo, C hi, C mod m, ~e}, C-sorted per class segment
    uint32_t *d_hoff = nullptr;        // hint CSR on the device (dump path)
    uint8_t *d_hbytes = nullptr;
    uint64_t max_seeds = 0;
    nmz::DevBuf seed_scratch;           // h0, buckets, sorted seeds
    nmz::DevBuf partial;                // per-chunk partial (sum, key) per seed
    nmz::DevBuf topk_lists;             // top-k selection scratch (nmz_replayable_sweep_topk_dev)
    nmz::DevBuf plan_mem;
    nmz::OqState oq;                    // order-query statistics (k_replayable_sweep_oq)
    nmz::WtState wt;                    // wavelet-tree statistics (k_replayable_sweep_wt, the default when it fits)
    nmz::DevBuf wt_topk;                // their top-k scratch (candidates, chunk records)
    // every pooled buffer of the plan: plan_create assigns their pool, plan_destroy_locked releases them
    std::array<nmz::DevBuf *, 8> buffers() {
        return {&plan_mem, &seed_scratch, &partial, &topk_lists, &oq.mem, &wt.mem, &wt.aux, &wt_topk};
    }
    // recorded on the context's stream after the plan's build: a sweep on another stream waits for it on the
    // device (nmz_replayable_plan_create_async returns before the build has run)
    hipEvent_t built = nullptr;
    // the streams the plan's sweeps were enqueued on, each with an event recorded after its latest sweep:
    // destroy waits for exactly that work and the build, not for the whole device or the context's stream
    struct Use {
        hipStream_t st;
        hipEvent_t ev;
    };
    std::vector<Use> uses;
};

// A prepared seed set (nmz_replayable_seeds_create): the seeds' prefix hashes, bucketed by row at the statistics
// kernels' granularity, and the row histogram (the per-decision sweeps bucket the hashes again at theirs)
struct nmz_replayable_seeds {
    nmz_ctx *ctx = nullptr;
    uint64_t S = 0;
    nmz::DevBuf mem;
    nmz::SeedScratch sc{};
    uint32_t *hist = nullptr;  // [bucket_hist_u32(S)] the prefix kernel's rows of bucket counts
};
