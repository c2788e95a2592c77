// K3 (edit distance) declarations shared by its translation units: the plan, the kernels' argument structs and the
// entry points of ed_build.hip (plan builders), ed_tp.hip (two-phase search), ed_bv.hip and ed_wide.hip (kernels).
// ed.hip holds k_ed_tile, the generic kernel, the k-NN list kernels, the search's dispatch and the C ABI. Also here:
// what ed_moves_wide.hip (K9w) takes from ed_align_wide.hip (K8w's host helpers) and shares with ed_moves.hip (K9),
// what ed_po.hip (K10) takes from both, and what ed_po_knn.hip (K11) takes from ed_po.hip. (The aligners' shared
// device pieces are ed_align_dev.h; their shared host side and PlanFence are declared in nmz_internal.h.)
#pragma once
#include <memory>
#include <string>
#include <unordered_map>

#include "nmz_common.h"
#include "nmz_internal.h"

namespace nmz {

constexpr uint16_t CAND_PAD = 0xffff;  // candidate symbol past its end (never a real id)
constexpr uint32_t MAX_FAST_LEN = 0x7000;
constexpr uint32_t MAX_FAST_SYMBOLS = 0xfffd;

// The shard that owns query block qb (64 queries) of the bit-parallel search, in both its forms (two-phase and the
// single kernel, so the pairs a shard owns do not depend on which form a rank's plan took): rotated snake order. A query block's
// work falls with qb inside the upper triangle (fewer candidates j > q) and inside every family of near-duplicates;
// in each period of 2S blocks, block r and its mirror 2S-1-r form pair min(r, 2S-1-r), so linear trends cancel, and
// the pair goes to shard (pair + period) mod S, so over the periods every shard takes every pair position. (A plain
// snake gives shard s the same two positions in every period: when the work's own period matches -- families of 16
// blocks at 8 shards -- shard 0 always held each family's first and last block, whose short candidate lists run the
// DP less efficiently (1.15x); the MurmurHash3 deal of round 2 left max/mean 1.15. DESIGN.md section 6.) A fixed
// rule, not a knob: one process per GPU computes its own shards' tiles, so the rule must be the same everywhere.
// (Dealing runs of 4 or 16 consecutive blocks instead, to keep a family's candidates in one shard's L2, measured
// worse: 8-shard sum / unsharded 1.17 / 1.16 clustered vs 1.14; profiles/r04/ed_deal_chunk_ab.)
__host__ __device__ inline uint32_t ed_block_shard(uint32_t qb, uint32_t n_shards) {
    if (n_shards <= 1) return 0;
    const uint32_t r = qb % (2 * n_shards), pr = r < n_shards ? r : 2 * n_shards - 1 - r;
    return (pr + qb / (2 * n_shards)) % n_shards;
}
bool ed_bv_supported(uint32_t band);   // band <= 64
uint32_t ed_bv_template(uint32_t band);  // the kernels' template band W >= band: 8, 16, 32 or 64
// LDS of one bit-parallel workgroup: the kernels with a pool (k_ed_bv, k_ed_bv_dp) stay within 64 KiB (several
// workgroups per CU); single queries (k_ed_bv_query, ~N / 256 workgroups) may take up to ED_BV_LDS_MAX
constexpr size_t ED_BV_LDS_MAX = 160 * 1024;

// bit-parallel banded edit distance (ed_bv.hip): 2 queries x a pool of ED_BV_POOL candidates per workgroup
constexpr uint32_t ED_BV_POOL = 1024;  // base pool; the plan scales it up to 4x for large N (ed_build.hip)
struct EdBvArgs {
    const uint16_t *bsym;         // per-trace streams of Peq-row byte offsets (u16), padded to 32-blocks + 1
    const uint64_t *soff;         // [N] element offset of each trace's stream
    const uint32_t *len;          // [N]
    const uint64_t *chunk_start;  // [G+1] this shard's first chunk of each 64-query block row (row b's chunks
                                  // cr = ((shard - b) mod n_shards) + n_shards * t, t = 0, 1, ...)
    uint64_t *knn;                // [N][k]
    uint64_t *counters;           // [ED_BV_NCOUNTERS] work counters (nmz_ed_plan_counters), or nullptr
    const uint4 *prof;            // [N][ED_QG_DW / 4] q-gram profiles (ed_qgram_profiles), or nullptr: no filter
    uint64_t n_chunks;            // chunks of this shard
    uint32_t N, G, k, lds_dw, shard, n_shards, pool;
    uint32_t w;                   // the requested band (<= the kernel's template W)
    // compact tables (CMP kernels): LDS dword offsets of the id -> row map (u16) and of the claim bitmap, and the
    // bytes per Peq row; lds_dw covers Peq rows + map + bitmap
    uint32_t rmap_dw, claim_dw, row_bytes;
    uint32_t rq;                  // queries per block row (64 x ED_BV_ROW_WAVES64); rq / 2 workgroups share a chunk
};
// Block rows of the bit-parallel search: rq = 64 * ED_BV_RW queries; the rq / 2 workgroups of one chunk (one query
// pair each, the same pool of candidates) are consecutive in the XCD-remapped order, so they run together on one
// XCD and read the pool's candidate streams from its L2. 5 x 32 = 160 workgroups = one XCD's 32 CUs x 5.
constexpr uint32_t ED_BV_RW = 5;
// k_ed_bv work counters, summed over the launch:
//   0 pairs that ran the DP, 1 pairs with a result <= w (in band), 2 lane-candidate 32-column blocks executed,
//   3 candidates that ran the DP, 4 live query-blocks (blocks x queries of that lane still running),
//   5 pairs inside the length band settled at w + 1 by the q-gram bound (no DP)
constexpr int ED_BV_NCOUNTERS = 6;
// the counters live in ED_CNT_STRIPES stripes of 16 u64 (one 128-byte line each); a wave adds to stripe
// (blockIdx mod ED_CNT_STRIPES) and nmz_ed_plan_counters sums the stripes (one address for the whole grid
// serialised ~10^6 same-address atomics: 10 ms of a 16 ms filter pass)
constexpr uint32_t ED_CNT_STRIPES = 64, ED_CNT_LINE = 16, ED_CNT_WORDS = ED_CNT_STRIPES * ED_CNT_LINE;
// q-gram (bigram) profiles: per trace, ED_QG_BUCKETS counts of hashed adjacent symbol pairs, saturated at 255 and
// packed 4 per dword. One edit changes at most 4 bigram counts by one, so ED >= L1(profile_a, profile_b) / 4
// (merging bigrams into buckets and saturating only lower the L1); L1 > 4w settles ED_w = w + 1 without a DP.
constexpr uint32_t ED_QG_BUCKETS = 128, ED_QG_DW = ED_QG_BUCKETS / 4;
int ed_qgram_profiles(const uint16_t *bs, const uint64_t *soff, const uint32_t *len, uint32_t N, uint32_t *prof,
                      hipStream_t st);
// Two-phase bit-parallel search (ed_bv.hip), used when the q-gram filter is on:
//   1. k_ed_qg_filter over tiles of 64 queries x 256 candidates (a candidate's profile in registers against 64
//      query profiles in LDS) decides every pair's length band and q-gram bound; a count pass sizes, and a write
//      pass fills, per query pair (2p, 2p + 1) a list of entries j | run1 << 30 | run2 << 31 (pairs needing a DP);
//   2. k_ed_bv_dp runs work items of <= `item` entries of one query pair each (its Peq tables in LDS);
//      ed_bv_item() picks the size (NMZ_ED_ITEM overrides, a power of two in [64, 4096]).
constexpr uint32_t ED_BV_ITEM = 4096;  // the largest item
struct EdQgArgs {
    const uint4 *prof;           // [N][ED_QG_DW / 4] q-gram profiles
    const uint32_t *len;         // [N]
    uint64_t *knn;               // [N][k]: in-band results decided here (an empty trace in the length band)
    uint64_t *counters;          // [ED_BV_NCOUNTERS] or nullptr (count pass only)
    const uint64_t *tiles;       // [n_tiles] this shard's tiles, qb << 32 | cb
    uint32_t *cnt;               // [n_pairs] entries per query pair: the count pass adds, the write pass takes
                                 // them back (its slots: poff[p] + the count left), so they end at zero again
    const uint32_t *poff;        // write pass: [n_pairs] the pairs' entry offsets
    uint32_t *ent;               // write pass: the entries
    uint4 *recs;                 // count pass: one record per (wave, query pair) with survivors -- {pair, first
                                 // candidate, run1 ballot} and {run2 ballot} (2 uint4) -- for the scatter pass, or
                                 // nullptr (the write pass recomputes the filter); ED_REC_STRIPES regions of rec_cap
    uint32_t *n_rec;             // [ED_REC_STRIPES * ED_REC_LINE] records appended per stripe (workgroup mod
                                 // ED_REC_STRIPES; one counter per 128-byte line: a single counter for the grid
                                 // serialised ~10^5-10^6 same-address atomics); past rec_cap the write pass recomputes
    const uint32_t *rec_cnt;     // scatter pass: [ED_REC_STRIPES] the count pass's records per stripe
    uint32_t rec_cap;            // records per stripe
    uint64_t n_tiles;
    uint32_t N, k, QB, NCB, shard, n_shards;
    uint32_t w;                  // band
    // write pass: the entry lists' capacity, and a device flag that, when set, makes the write pass (and the DP,
    // ed_bv_dp_launch's `abort`) skip: a search enqueued with a shard's cached sizes whose own totals differ
    // (k_tp_scan sets it) must not write past lists sized for the cached totals
    uint64_t ent_cap;
    const uint32_t *abort;
};
constexpr uint32_t ED_REC_STRIPES = 64, ED_REC_LINE = 32;
int ed_qg_filter_launch(const EdQgArgs &A, bool count, hipStream_t st);
int ed_qg_scatter_launch(const EdQgArgs &A, uint32_t n_rec, hipStream_t st);
int ed_bv_dp_launch(const EdBvArgs &A, const uint32_t *ioff, const uint32_t *poff, const uint32_t *ent,
                    uint32_t n_pairs, uint32_t n_items, uint32_t item, uint32_t bw, bool cmp, hipStream_t st,
                    const uint32_t *abort = nullptr);
// single-query search on a bit-parallel plan (ed_bv.hip k_ed_bv_query): 1-2 external queries vs every stored trace
struct EdBvQueryArgs {
    const uint16_t *bsym;  // the plan's stored streams
    const uint64_t *soff;
    const uint32_t *len;
    const uint16_t *qs;    // query streams (plan's Peq-row byte offsets; 0xffff = symbol unknown to the store)
    uint64_t qoff[2];
    uint32_t nq[2];
    uint64_t *knn;         // [n_queries][k]
    const uint4 *prof;     // the stored traces' q-gram profiles, or nullptr: no filter
    uint32_t N, k, lds_dw, pool, n_queries;
    uint32_t w, rmap_dw, claim_dw, row_bytes;  // band; compact tables as in EdBvArgs
};
int ed_bv_query_launch(const EdBvQueryArgs &A, uint32_t bw, bool cmp, uint32_t blocks, hipStream_t st);
int ed_bv_launch(const EdBvArgs &A, uint32_t bw, bool cmp, uint64_t blocks, hipStream_t st);

// wide-band bit-parallel edit distance (ed_wide.hip): one pair per wave
struct EdWideArgs {
    const uint16_t *sym;   // dense symbol ids, CSR order (padded with 64 zeros)
    const uint64_t *off;   // [N+1]
    const uint32_t *rowb;  // per trace, per position: byte offset of that symbol's Peq row (c * ndw * 4),
                           // each trace starting at a multiple of 32 entries, padded by >= 64 zero entries
    const uint64_t *rowb_off;  // [N]: first entry of trace j in rowb
    const uint32_t *peq;   // [N][n_sym][ndw] match bitmaps
    uint64_t *knn;         // [N][k]
    uint64_t n_pairs;      // N(N-1)/2
    uint64_t n_waves;      // waves of this shard (chunks of 32 pairs dealt round-robin)
    uint32_t N, k, n_sym, ndw, shard, n_shards;
    uint32_t w;            // the requested band (<= the kernel's W)
};
bool ed_wide_supported(uint32_t band);   // 64 < band <= 8192
uint32_t ed_wide_template(uint32_t band);  // W = 1024, 2048, 4096 or 8192 >= band
uint32_t ed_wide_ndw(uint32_t band, uint32_t max_len);
int ed_wide_build_peq(const uint16_t *d_sym, const uint64_t *d_off, uint32_t N, uint32_t n_sym, uint32_t ndw,
                      uint32_t band, uint32_t *d_peq, hipStream_t st);
int ed_wide_launch(const EdWideArgs &A, uint32_t band, hipStream_t st);
// single queries: wave (q, j) over n_q query tables qpeq + q * qstride (rows over the store's alphabet) x the N
// stored traces of A; in-band results into A.knn + q * k
int ed_wide_query_launch(const EdWideArgs &A, uint32_t band, const uint32_t *qpeq, uint64_t qstride,
                         const uint32_t *qlen, uint32_t n_q, hipStream_t st);

// ---- edit scripts over wide bands (ed_align_wide.hip), for ed_moves_wide.hip ----
// aw_validate: every limit of nmz_ed_align_wide_pairs, no device; *max_len = the longest trace of the pairs.
// aw_shape: the plan's shape for (band, max_len), no device. The _locked forms and aw_enqueue want the caller to
// hold the context.
int aw_band(uint32_t band);
int aw_validate(const uint64_t *off, const uint64_t *sym, uint32_t n_traces, const uint32_t *pairs, uint64_t n_pairs,
                uint32_t band, const uint32_t *dist, const nmz_edit_op *ops, uint64_t *max_len);
int aw_shape(uint32_t band, uint64_t max_len, uint64_t *slot_words);
int aw_plan_create_locked(nmz_ctx *ctx, uint32_t band, uint64_t max_len, uint64_t slot_words,
                          nmz_ed_align_wide_plan **out);
void aw_plan_destroy_locked(nmz_ed_align_wide_plan *p);
int aw_enqueue(nmz_ed_align_wide_plan *p, hipStream_t st, const uint64_t *d_off, const uint64_t *d_sym,
               const uint32_t *d_pairs, uint64_t n_pairs, uint32_t *d_dist, nmz_edit_op *d_ops);

// ---- move profiles: what K9 (ed_moves.hip) and K9w (ed_moves_wide.hip) share ----
constexpr uint64_t MV_LDS_SYMS = 2048;  // the table is staged in LDS up to this size (16 KiB)
constexpr uint64_t MV_MISS = ~0ull;

struct MvArgs {
    const uint64_t *off, *sym;
    const uint32_t *pairs;
    uint64_t n_pairs;
    uint32_t band;
    const uint32_t *dist;
    const nmz_edit_op *ops;
    const uint64_t *usym;
    uint64_t n_usym;
    uint32_t *partner;  // may be NULL
    nmz_move_counts *counts;
    nmz_move_info *info;
};

// index of v in the strictly increasing tab[U], MV_MISS if absent; the trip count depends on U alone
__device__ __forceinline__ uint64_t mv_find(const uint64_t *tab, uint64_t U, uint64_t v) {
    if (U == 0) return MV_MISS;
    uint64_t lo = 0, n = U;
    while (n > 1) {
        const uint64_t h = n >> 1;
        lo = tab[lo + h] <= v ? lo + h : lo;
        n -= h;
    }
    return tab[lo] == v ? lo : MV_MISS;
}

// the band check and the aligner's validator of a profile form: align_band / align_validate (band <= 64) or
// aw_band / aw_validate (band <= 1,024)
typedef int (*MvBandCheck)(uint32_t band);
typedef int (*MvAlignValidate)(const uint64_t *off, const uint64_t *sym, uint32_t n_traces, const uint32_t *pairs,
                               uint64_t n_pairs, uint32_t band, const uint32_t *dist, const nmz_edit_op *ops,
                               uint64_t *max_len);
// one live op against its traces
int moves_op_check(const nmz_edit_op &o, uint64_t n, uint64_t m, const std::string &where);
// every limit of the host-pointer profile forms, no device. ops == nullptr with want_ops == false: the scripts are
// made on the device (nmz_ed_diff_profile*)
int moves_validate(MvBandCheck band_ok, MvAlignValidate validate, const uint64_t *off, const uint64_t *sym,
                   uint32_t n_traces, const uint32_t *pairs, uint64_t n_pairs, uint32_t band, const uint32_t *dist,
                   const nmz_edit_op *ops, bool want_ops, const uint64_t *usym, uint64_t n_usym,
                   const nmz_move_counts *counts, const nmz_move_info *info, uint64_t *max_len);
// partner[n_ops] by the definition; the ops are live and inside their traces
void moves_partners(const uint64_t *a, const uint64_t *b, const nmz_edit_op *ops, uint32_t n_ops, uint32_t *partner);
void moves_zero(nmz_move_counts *counts, uint64_t n_usym, nmz_move_info *info);
// the body of nmz_move_profile_host and nmz_move_profile_wide_host: the whole profile on the calling thread
int moves_profile_host(MvBandCheck band_ok, MvAlignValidate validate, const uint64_t *off, const uint64_t *sym,
                       uint32_t n_traces, const uint32_t *pairs, uint64_t n_pairs, uint32_t band, const uint32_t *dist,
                       const nmz_edit_op *ops, const uint64_t *usym, uint64_t n_usym, uint32_t *partner,
                       nmz_move_counts *counts, nmz_move_info *info);
// K9's launch (band <= 64) behind its argument checks and the clear; the caller holds the context
int moves_enqueue(nmz_ctx *ctx, hipStream_t st, const MvArgs &a, int accumulate);
// K9w's launch (every band 0 .. 1,024; ed_moves_wide.hip), for ed_po.hip; the caller holds the context
int moves_wide_enqueue(nmz_ctx *ctx, hipStream_t st, const MvArgs &a, int accumulate);


// ---- the projection of ed_po.hip (K10a, the scan, K10b), for ed_po_knn.hip (K11); the caller holds the context ----
int po_project_enqueue(nmz_ctx *ctx, hipStream_t st, const uint64_t *d_off, const uint64_t *d_sym,
                       const uint32_t *d_ent, uint32_t n_traces, uint32_t G, uint64_t *d_poff, uint64_t *d_psym,
                       uint32_t *d_psrc);

}  // namespace nmz

// ED plan: symbol remap + device layouts (reused across searches)
struct nmz_ed_plan {
    nmz_ctx *ctx = nullptr;
    uint32_t n = 0, band = 0, G = 0;
    bool fast = false;
    bool bv = false;               // bit-parallel kernel (k_ed_bv) usable
    uint64_t *d_soff = nullptr;    // bv: per-trace stream offsets
    uint32_t pool = 0;
    bool wide = false;             // wide-band bit-parallel kernel (k_ed_wide) usable
    bool tile = false;             // k_ed_tile (dense ids in d_qsym / d_qoff)
    uint32_t n_sym = 0;
    uint32_t *d_peq = nullptr;     // wide: [N][n_sym][ndw] match bitmaps
    uint32_t *d_rowb = nullptr;    // wide: per-position Peq row byte offsets (EdWideArgs::rowb)
    uint64_t *d_rowb_off = nullptr;
    uint32_t ndw = 0, lds_dw = 0;  // bv: dwords per Peq row per query, LDS dwords per workgroup
    uint64_t n_chunks = 0;         // bv: total chunks (64-query block row x ED_BV_POOL candidates)
    uint16_t *d_bsym = nullptr;
    uint64_t *d_chunk_start = nullptr;  // bv: [G+1] per-row chunk starts (single-kernel search)
    uint64_t *d_counters = nullptr;  // bv: work counters of the latest search (nmz_ed_plan_counters)
    uint32_t *d_prof = nullptr;      // bv: [N][ED_QG_DW] q-gram profiles (ed_qgram_profiles)
    uint32_t rq = 64;                // bv: queries per block row
    uint32_t maxlen = 0;
    uint32_t bw = 0;                 // bv: the kernels' template band W >= band (8, 16, 32, 64)
    bool cmp = false;                // bv: compact tables (streams of symbol ids, per-workgroup rows; ed_bv.hip)
    uint32_t rmap_dw = 0, claim_dw = 0, row_bytes = 0;  // bv, compact: LDS layout (EdBvArgs)
    uint32_t ww = 0;                 // wide: the kernel's W (1024 * 2^k >= band)
    std::unordered_map<uint64_t, uint32_t> dict;  // bv: symbol -> dense id (single-query search)
    nmz::DevBuf mem;
    // bv, two-phase search: per-(shard, n_shards) tile starts (host, kept), scratch and the entry lists
    std::map<uint64_t, nmz::DevBuf> tile_list;      // per (shard, n_shards): the shard's tiles (qb << 32 | cb)
    std::map<uint64_t, uint64_t> tile_count;
    nmz::DevBuf tp_mem, tp_ent, tp_rec;
    struct TpSizes {
        uint64_t tot64;
        uint32_t items, n_rec, item;
    };
    std::map<uint64_t, TpSizes> tp_sizes;  // per (shard, n_shards): entry total, DP items, records of its searches
    uint32_t *d_tp_mismatch = nullptr;     // (in tp_mem) set when a search's totals differ from tp_sizes
    uint64_t tp_mem_gen = 0, tp_rec_gen = 0;  // DevBuf::gen of tp_mem / tp_rec when their counters were last cleared
    bool tp_dirty = false;                 // a count pass's counts not yet taken back by its write pass
    // the mismatch flag as of the last search enqueued with cached sizes: that search's offsets scan writes {its
    // sequence number, the flag} to these pinned words, read (ed_tp_flag_check) by the shard's next search without
    // waiting once the number has landed, or read from the device with a wait by the synchronous entry points
    // (nmz_ed_plan_counters, the group search)
    uint32_t *h_tp_flag = nullptr;
    uint32_t tp_seq = 0;       // the latest cached search's number
    uint32_t tp_seq_sent = 0;  // the latest number whose scan was enqueued (the last writer of h_tp_flag)
    bool tp_flag_armed = false;
    // fixed at creation (NMZ_ED_QGRAM / NMZ_ED_TWO_PHASE, A/B knobs read once per plan), so every shard and every
    // call of one plan takes the same search and deals pairs by the same rule
    bool qgram = true, two_phase = true;
    uint32_t opts = 0;               // NMZ_ED_OPT_* the plan was created with (options | A/B knobs)
    uint64_t total = 0, off_hash = 0;  // symbols in the store; FNV-1a of its offsets (nmz_ed_plan_fingerprint)
    uint16_t *d_qsym = nullptr, *d_csym = nullptr;
    uint64_t *d_qoff = nullptr, *d_coff = nullptr;
    uint32_t *d_gmax = nullptr, *d_len = nullptr;
    // generic path
    uint64_t *d_off64 = nullptr, *d_sym64 = nullptr;
};

namespace nmz {

// RAII: a scratch DevBuf of one call goes back when the call returns, on every path
struct ScopedRelease {
    DevBuf &b;
    ~ScopedRelease() { b.release(); }
};

// ---- the plan's owner (ed_build.hip) ----
// The one place a plan is released: its pooled buffers, the tile lists, the pinned flag words (ed_tp_flag_release
// waits for their last writer), then the plan itself. The caller holds the plan's context.
void ed_plan_release(nmz_ed_plan *p);
struct EdPlanDelete {
    void operator()(nmz_ed_plan *p) const { ed_plan_release(p); }
};
typedef std::unique_ptr<nmz_ed_plan, EdPlanDelete> EdPlanPtr;
// d_sym: the symbols on the device instead of sym (host); the host build paths take a copy of them
int ed_plan_build(nmz_ctx *ctx, const uint64_t *off, const uint64_t *sym, uint32_t N, uint32_t band,
                  nmz_ed_plan **out, const uint64_t *d_sym = nullptr, uint32_t opts = 0);
// Compact bit-parallel tables (ed_bv.hip CMP): R rows for a workgroup's queries + the zero row, the map of
// n_ids symbol ids (+ the padding id) to row byte offsets (u16), the claim bitmap. False when they do not fit
// `limit` bytes with `extras` (or a row offset would not fit 16 bits).
bool bv_compact_layout(uint32_t n_ids, uint32_t R, uint32_t ndw, size_t extras, size_t limit, uint32_t &lds_dw,
                       uint32_t &rmap_dw, uint32_t &claim_dw);

// ---- the two-phase bit-parallel search (ed_tp.hip) ----
// the cached-size mismatch flag: wait = synchronise `st` and read it; otherwise read the last search's pinned copy
// if it has landed. Fails (and resets the flag and the cache) when it is set.
int ed_tp_flag_check(nmz_ed_plan *p, bool wait, hipStream_t st);
void ed_tp_flag_release(nmz_ed_plan *p);
// one shard's search into d_knn; 1 when the plan cannot take it at all (the caller runs the single kernel)
int ed_bv_two_phase(nmz_ed_plan *p, hipStream_t st, EdBvArgs &A, uint64_t *d_knn);

// ---- the k-NN list kernels (ed.hip) for the other files; errors surface at the caller's next hipGetLastError ----
void knn_init_launch(uint64_t *knn, uint64_t n, hipStream_t st);
void knn_fill_launch(uint64_t *knn, uint32_t n_lists, uint32_t k, uint32_t n_cand, uint32_t fill_d, int self_exclude,
                     hipStream_t st);
// a search's end: the lists' ids and distances (k_knn_final into d_id, d_ds) copied to the host; synchronises st
int knn_final_to_host(HostCall &call, const uint64_t *knn, uint64_t n, uint32_t *d_id, uint32_t *d_ds,
                      uint32_t *knn_id, uint32_t *knn_dist);

// the EdWideArgs fields a wide plan fixes: its store, its tables, one shard; the caller adds the lists and the waves
inline EdWideArgs ed_wide_plan_args(const nmz_ed_plan *p, uint32_t k) {
    EdWideArgs A;
    A.sym = p->d_qsym;
    A.off = p->d_qoff;
    A.rowb = p->d_rowb;
    A.rowb_off = p->d_rowb_off;
    A.peq = p->d_peq;
    A.N = p->n;
    A.k = k;
    A.n_sym = p->n_sym;
    A.ndw = p->ndw;
    A.shard = 0;
    A.n_shards = 1;
    A.w = p->band;
    return A;
}

}  // namespace nmz
