// K3b's two-phase search, host side (kernels: ed_bv.hip; ed_plan.h EdQgArgs). Per shard: a filter count pass over the
// shard's tiles, the offsets scan (k_tp_reduce, k_tp_scan), the write pass, the DP over the work items. A shard's
// first search reads the totals back; later ones run with the cached sizes, guarded by the mismatch flag.
#include <algorithm>
#include <chrono>
#include <thread>

#include "ed_plan.h"

namespace nmz {

// Entries per DP work item. One workgroup runs one item with its pair's Peq tables; the last items of a launch
// leave CUs idle until they end, so their length is the launch's tail (~1 item per CU slot): a shard of the
// 8-GPU search has 1/8 of the items, so the tail weighs 8x more there.
static uint32_t ed_bv_item() {
    if (const char *e = ab_env("NMZ_ED_ITEM")) {
        const uint32_t v = (uint32_t)atoi(e);
        if (v >= 64 && v <= ED_BV_ITEM && (v & (v - 1)) == 0) return v;
    }
    return ED_BV_ITEM;
}

// The item size of a search with n_ent DP entries: about ED_DP_ITEMS_TARGET items (8 per workgroup slot of the
// chip), a power of two in [128, ED_BV_ITEM]. Large items keep every lane busy (a lane refills from its item's
// entries as its pairs end); small ones shorten the last round of a launch, which dominates a shard's search when
// its entries are few (configs[2], 8 shards, item 4096 -> 256: clustered shard DP 9.75 -> 9.45 ms, survey 0.41-0.62
// -> 0.35-0.41 ms, profiles/r05/ed_item_ab). An NMZ_ED_ITEM setting (A/B) wins.
constexpr uint64_t ED_DP_ITEMS_TARGET = 8ull * 256 * 5;
static uint32_t ed_bv_pick_item(uint64_t n_ent) {
    if (ab_env("NMZ_ED_ITEM")) return ed_bv_item();
    uint32_t it = 128;
    while (it < ED_BV_ITEM && (uint64_t)it * 2 * ED_DP_ITEMS_TARGET <= n_ent) it *= 2;
    return it;
}

// the largest entry list of one batch, and the survivor records' bytes
constexpr uint64_t ED_TP_MAX_ENTRIES = 1ULL << 30;  // 4 GiB of entries
constexpr uint64_t ED_TP_MAX_REC_BYTES = 1ULL << 30;

// the entry-list limit (NMZ_ED_TP_MAX_ENTRIES lowers it, so tests can force the single-kernel fallback)
static uint64_t ed_tp_max_entries() {
    if (const char *e = ab_env("NMZ_ED_TP_MAX_ENTRIES")) {
        const unsigned long long v = strtoull(e, nullptr, 10);
        if (v < ED_TP_MAX_ENTRIES) return v;
    }
    return ED_TP_MAX_ENTRIES;
}

// The two-phase search's offsets after a count pass (ed_bv_two_phase), in two launches: k_tp_reduce sums each
// block's chunk of query pairs (DP entries, work items of `item` entries), k_tp_scan turns the sums into the pairs'
// entry offsets (poff) and work-item offsets (ioff). The last block writes the 64-bit entry total (the u32 offsets
// wrap beyond 2^32 entries, so they are trusted only while the total is within the batching limit), compares the
// totals with a shard's cached sizes (flag), and moves the survivor-record counter to rec_out, leaving it at zero
// for the next count pass. (These were hipcub scans of the two arrays, an item kernel, a one-block sum, a verify
// kernel, a cursor copy and two clears: 11 launches and ~55 us per search, a fixed cost each shard of the 8-GPU
// search paid once more.)
constexpr uint32_t TP_PER_THREAD = 8, TP_TILE = 256 * TP_PER_THREAD, TP_MAX_BLOCKS = 256;
struct TpScanArgs {
    const uint32_t *cnt;    // [n] DP entries per query pair
    uint32_t n, lg_item;    // pairs; log2 entries per work item
    uint32_t chunk, nb;     // pairs per block (a multiple of TP_TILE), blocks (<= TP_MAX_BLOCKS)
    uint64_t *agg;          // [2 TP_MAX_BLOCKS]: block b's entries, items
    uint32_t *poff, *ioff;  // [n + 1]
    uint64_t *tot64;
    uint32_t *n_rec, *rec_out;  // the records' stripe counters (or nullptr) and where their total goes (UINT32_MAX
                                // when a stripe overflowed rec_share: the write pass then recomputes)
    uint32_t *rec_cnt;          // [ED_REC_STRIPES] the stripes' counts, for the scatter
    uint32_t rec_share;
    uint32_t *flag;         // or nullptr: no cached sizes to compare
    uint64_t e_tot;
    uint32_t e_items, e_rec;
    uint32_t *h_flag;       // with flag: pinned host words {seq, flag} the check publishes (ed_tp_flag_check)
    uint32_t seq;
};

__device__ __forceinline__ uint32_t tp_items(uint32_t c, uint32_t lg) { return (c + (1u << lg) - 1) >> lg; }

// block-wide sums of two u64 (256 threads); every thread gets them
__device__ __forceinline__ void tp_block_sum(uint64_t &a, uint64_t &b, uint64_t (*sh)[4]) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        a += __shfl_xor((unsigned long long)a, off, 64);
        b += __shfl_xor((unsigned long long)b, off, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        sh[0][threadIdx.x >> 6] = a;
        sh[1][threadIdx.x >> 6] = b;
    }
    __syncthreads();
    a = sh[0][0] + sh[0][1] + sh[0][2] + sh[0][3];
    b = sh[1][0] + sh[1][1] + sh[1][2] + sh[1][3];
    __syncthreads();
}

__global__ __launch_bounds__(256) void k_tp_reduce(TpScanArgs A) {
    __shared__ uint64_t sh[2][4];
    const uint32_t lo = blockIdx.x * A.chunk, hi = min(A.n, lo + A.chunk);
    uint64_t e = 0, it = 0;
    for (uint32_t i = lo + threadIdx.x; i < hi; i += 256) {
        const uint32_t c = A.cnt[i];
        e += c;
        it += tp_items(c, A.lg_item);
    }
    tp_block_sum(e, it, sh);
    if (threadIdx.x == 0) {
        A.agg[2 * blockIdx.x] = e;
        A.agg[2 * blockIdx.x + 1] = it;
    }
}

__global__ __launch_bounds__(256) void k_tp_scan(TpScanArgs A) {
    __shared__ uint64_t sh[2][4];
    const uint32_t t = threadIdx.x, lane = t & 63, wv = t >> 6;
    uint64_t ce = 0, ci = 0;  // the entries and items before this block (nb <= 256: one sum per thread)
    if (t < blockIdx.x) {
        ce = A.agg[2 * t];
        ci = A.agg[2 * t + 1];
    }
    tp_block_sum(ce, ci, sh);
    const uint32_t hi = min(A.n, (blockIdx.x + 1) * A.chunk);
    for (uint32_t base = blockIdx.x * A.chunk; base < hi; base += TP_TILE) {
        const uint32_t i0 = base + TP_PER_THREAD * t;
        uint32_t c[TP_PER_THREAD];
        if (i0 + TP_PER_THREAD <= hi) {
            const uint4 x = *(const uint4 *)(A.cnt + i0), y = *(const uint4 *)(A.cnt + i0 + 4);
            c[0] = x.x, c[1] = x.y, c[2] = x.z, c[3] = x.w, c[4] = y.x, c[5] = y.y, c[6] = y.z, c[7] = y.w;
        } else {
#pragma unroll
            for (uint32_t k = 0; k < TP_PER_THREAD; ++k) c[k] = i0 + k < hi ? A.cnt[i0 + k] : 0u;
        }
        uint64_t se = 0, si = 0;
#pragma unroll
        for (uint32_t k = 0; k < TP_PER_THREAD; ++k) {
            se += c[k];
            si += tp_items(c[k], A.lg_item);
        }
        // the thread's exclusive prefix inside the tile: wave scan, then the earlier waves' totals
        uint64_t xe = se, xi = si;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint64_t ue = __shfl_up((unsigned long long)xe, d, 64), ui = __shfl_up((unsigned long long)xi, d, 64);
            if (lane >= (uint32_t)d) {
                xe += ue;
                xi += ui;
            }
        }
        if (lane == 63) {
            sh[0][wv] = xe;
            sh[1][wv] = xi;
        }
        __syncthreads();
        uint64_t pe = ce + xe - se, pi = ci + xi - si, te = 0, ti = 0;
        for (uint32_t w = 0; w < 4; ++w) {
            if (w < wv) {
                pe += sh[0][w];
                pi += sh[1][w];
            }
            te += sh[0][w];
            ti += sh[1][w];
        }
        __syncthreads();
#pragma unroll
        for (uint32_t k = 0; k < TP_PER_THREAD; ++k) {
            if (i0 + k < hi) {
                A.poff[i0 + k] = (uint32_t)pe;
                A.ioff[i0 + k] = (uint32_t)pi;
            }
            pe += c[k];
            pi += tp_items(c[k], A.lg_item);
        }
        ce += te;
        ci += ti;
    }
    if (blockIdx.x + 1 == A.nb && t < 64) {  // the last block's first wave: totals, record counts, the check
        uint32_t r = 0;
        bool over = false;
        if (A.n_rec) {  // (ED_REC_STRIPES == 64: a lane per stripe)
            const uint32_t c = A.n_rec[t * ED_REC_LINE];
            A.rec_cnt[t] = c;
            A.n_rec[t * ED_REC_LINE] = 0;
            over = __ballot(c > A.rec_share) != 0;
            r = c;
            for (int o = 32; o >= 1; o >>= 1) r += __shfl_xor(r, o, 64);
            if (over) r = 0xFFFFFFFFu;
        }
        if (t == 0) {
            A.poff[A.n] = (uint32_t)ce;
            A.ioff[A.n] = (uint32_t)ci;
            *A.tot64 = ce;
            if (A.n_rec) *A.rec_out = r;
            if (A.flag) {
                if (ce != A.e_tot || (uint32_t)ci != A.e_items || r != A.e_rec) atomicOr(A.flag, 1u);
                // the device flag as it now stands (sticky until reported) to the host, then the search's sequence
                // number: the host reads the flag once it sees the number (no copy, no event on the queue)
                if (A.h_flag) {
                    const uint32_t fv = __hip_atomic_load(A.flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    __hip_atomic_store(A.h_flag + 1, fv, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                    __hip_atomic_store(A.h_flag, A.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
                }
            }
        }
    }
}

static int tp_offsets(TpScanArgs &A, uint32_t item, hipStream_t st) {
    A.lg_item = 0;
    while ((1u << A.lg_item) < item) ++A.lg_item;
    NMZ_CHECK((1u << A.lg_item) == item, "internal: the work-item size is not a power of two");
    const uint32_t tiles = (A.n + TP_TILE - 1) / TP_TILE;
    A.nb = std::min(tiles, TP_MAX_BLOCKS);
    A.chunk = (tiles + A.nb - 1) / A.nb * TP_TILE;
    A.nb = (A.n + A.chunk - 1) / A.chunk;
    hipLaunchKernelGGL(k_tp_reduce, dim3(A.nb), dim3(256), 0, st, A);
    hipLaunchKernelGGL(k_tp_scan, dim3(A.nb), dim3(256), 0, st, A);
    NMZ_HIP(hipGetLastError());
    return NMZ_OK;
}

// The mismatch flag of searches enqueued with a shard's cached sizes (see ed_bv_two_phase). Such a search's offsets
// scan compares its totals with the cache, sets the device flag on a difference and writes {its sequence number, the
// flag as it now stands} to pinned host words (no copy or event on the queue: each was ~5-10 us per search), and the
// plan is marked armed. check: read the host words -- without waiting (the shard's next search: a number
// not yet landed is read by a later call, the device flag stays set until reported) -- or the device flag after
// synchronising `st` (wait: the synchronous entry points); when set, clear it, drop every cached size (the next
// search recounts) and fail.
static int ed_tp_flag_host(nmz_ed_plan *p) {
    if (!p->h_tp_flag) {
        NMZ_HIP(hipHostMalloc((void **)&p->h_tp_flag, 8, hipHostMallocCoherent));  // device stores reach it directly
        p->h_tp_flag[0] = p->h_tp_flag[1] = 0;
        p->tp_seq = 0;
    }
    return NMZ_OK;
}

// the scan of search number `seq` has published its flag
static bool ed_tp_flag_landed(const nmz_ed_plan *p, uint32_t seq) {
    return __atomic_load_n(&p->h_tp_flag[0], __ATOMIC_ACQUIRE) == seq;
}

int ed_tp_flag_check(nmz_ed_plan *p, bool wait, hipStream_t st) {
    if (!p->d_tp_mismatch) return NMZ_OK;
    uint32_t f = 0;
    if (wait) {
        NMZ_HIP(hipMemcpyAsync(&f, p->d_tp_mismatch, 4, hipMemcpyDeviceToHost, st));
        NMZ_HIP(hipStreamSynchronize(st));
    } else {
        if (!p->tp_flag_armed || !p->h_tp_flag) return NMZ_OK;
        if (!ed_tp_flag_landed(p, p->tp_seq)) return NMZ_OK;  // not yet: a later call reads it (the flag stays set)
        f = __atomic_load_n(&p->h_tp_flag[1], __ATOMIC_ACQUIRE);
    }
    p->tp_flag_armed = false;
    if (!f) return NMZ_OK;
    NMZ_HIP(hipMemsetAsync(p->d_tp_mismatch, 0, 4, st));
    if (p->h_tp_flag) p->h_tp_flag[1] = 0;
    p->tp_sizes.clear();
    p->tp_dirty = true;  // the skipped write pass left the count pass's counts in place
    return fail(NMZ_EHIP, "internal: a two-phase search's totals differed from the shard's cached sizes; that search "
                          "wrote no entries and ran no DP (its k-NN lists are incomplete), and the cached sizes are "
                          "dropped");
}

// before the pinned flag words are freed: the last armed search's scan has written them (bounded wait, then a device
// synchronisation)
void ed_tp_flag_release(nmz_ed_plan *p) {
    if (!p->h_tp_flag) return;
    if (const uint32_t seq = p->tp_seq_sent) {
        for (int i = 0; i < 200000 && !ed_tp_flag_landed(p, seq); ++i)
            std::this_thread::sleep_for(std::chrono::microseconds(50));
        if (!ed_tp_flag_landed(p, seq)) (void)hipDeviceSynchronize();
    }
    (void)hipHostFree(p->h_tp_flag);
    p->h_tp_flag = nullptr;
}

// Tiles in 2-D superblocks of ED_SQ query blocks x ED_SC candidate blocks (2,048 queries x 4,096 candidates: 768
// KiB of profiles) and the filter kernels hand each XCD a contiguous range of the list, so an XCD's L2 holds a
// superblock's profiles while its tiles run (query-block order fetched every candidate profile once per query
// block: 7.1 GB per launch). Batches are whole groups of ED_SQ of the shard's query blocks.
constexpr uint32_t ED_SQ = 32, ED_SC = 16;

// the tiles (qb << 32 | cb) of the query blocks qbs[i0, i1), i0 < i1, in superblock order: their number, and the
// tiles themselves appended to *tiles when given
static uint64_t superblock_tiles(const std::vector<uint32_t> &qbs, size_t i0, size_t i1, uint32_t NCB,
                                 std::vector<uint64_t> *tiles) {
    uint64_t t = 0;
    for (uint32_t cb0 = qbs[i0] / 4; cb0 < NCB; cb0 += ED_SC)
        for (size_t i = i0; i < i1; ++i)
            for (uint32_t cb = std::max(cb0, qbs[i] / 4); cb < std::min(NCB, cb0 + ED_SC); ++cb, ++t)
                if (tiles) tiles->push_back(((uint64_t)qbs[i] << 32) | cb);
    return t;
}

// A shard's query blocks (qbs) and their groups of ED_SQ (grp: per group, its first index into qbs and its first tile).
// Every tile of query block qb belongs to shard ed_block_shard(qb). Whole query blocks, so a query pair's DP entries
// stay in one shard's work items: dealt by tile, a pair's near-duplicate candidates (a few 256-wide tiles) spread
// over several shards, every shard built the pair's Peq tables for a fraction of its entries, and the 8 shards
// summed to 1.15x the unsharded search. The DP work is data-dependent and clustered (the clustered workload's
// families put it next to the diagonal, with a period of 16 query blocks); a hash breaks that periodicity, where a
// round-robin deal aligned with it (8 shards: max/mean shard time 1.27)
static void shard_tiles(uint32_t QB, uint32_t NCB, uint32_t shard, uint32_t n_shards, std::vector<uint32_t> &qbs,
                        std::vector<uint32_t> &grp, std::vector<uint64_t> *tiles) {
    uint64_t t = 0;
    for (uint32_t qb = 0; qb < QB; ++qb)
        if (ed_block_shard(qb, n_shards) == shard) qbs.push_back(qb);
    for (size_t g0 = 0; g0 < qbs.size(); g0 += ED_SQ) {
        grp.push_back((uint32_t)g0);
        grp.push_back((uint32_t)t);
        t += superblock_tiles(qbs, g0, std::min(qbs.size(), g0 + ED_SQ), NCB, tiles);
    }
}

// One search of one shard: its scratch, the filter's arguments, and the passes that carry state across each other
// (the count pass's totals size the write pass and the DP; the item size fixes the offsets)
struct TpSearch {
    nmz_ed_plan *p;
    hipStream_t st;
    const EdBvArgs &A;
    EdQgArgs Q{};  // (no entries, no records until setup and write_dp give them)
    uint32_t n_pairs;
    uint32_t *f;  // {mismatch flag, record count out}
    uint64_t *d_tot64, *d_agg;
    uint32_t *d_rec_cnt, *d_cnt, *d_poff, *d_ioff;
    uint64_t rec_total_cap;  // records in the regions (UINT32_MAX records: a stripe overflowed its region)
    uint32_t item;           // entries per DP work item
    // the latest count pass's totals, read back (or taken from the shard's cached sizes)
    uint64_t tot64 = 0;
    uint32_t tot_items = 0, n_rec = 0;

    int setup(uint64_t n_tiles_all) {
        const uint32_t N = p->n;
        n_pairs = (N + 1) / 2;
        // scratch: {mismatch flag, record count out}, the entry total, the offset kernels' block sums, the records'
        // per-stripe counts, the per-pair counts (zero between searches: the write pass takes back what the count pass
        // added) and offsets
        ScratchLayout lay;
        lay.add(&f, 4).add(&d_tot64, 1).add(&d_agg, 2 * TP_MAX_BLOCKS).add(&d_rec_cnt, ED_REC_STRIPES);
        lay.add(&d_cnt, n_pairs + 1).add(&d_poff, n_pairs + 1).add(&d_ioff, n_pairs + 1);
        // an earlier search of this plan whose sizes contradicted the cache is reported here (without waiting for it)
        NMZ_TRY(ed_tp_flag_check(p, false, st));
        NMZ_TRY(lay.bind(p->tp_mem));
        if (p->tp_mem.gen != p->tp_mem_gen || f != p->d_tp_mismatch) {  // a new scratch buffer: flag and counts clear
            NMZ_HIP(hipMemsetAsync(p->tp_mem.ptr, 0, lay.bytes(), st));
            p->d_tp_mismatch = f;
            p->tp_mem_gen = p->tp_mem.gen;
        } else if (p->tp_dirty) {  // an earlier search stopped between its count and write passes
            NMZ_HIP(hipMemsetAsync(d_cnt, 0, (n_pairs + 1) * 4, st));
        }
        Q.prof = A.prof;
        Q.len = A.len;
        Q.knn = A.knn;
        Q.counters = A.counters;
        Q.cnt = d_cnt;
        Q.poff = d_poff;
        Q.abort = f;  // the mismatch flag: the write pass and the DP skip when it is set
        // the count pass's survivor records (32 B per (wave, query pair) with survivors) let the write pass scatter
        // without recomputing the filter; room for 16 per tile, in ED_REC_STRIPES equal regions (a stripe that overflows
        // its region: the write pass recomputes)
        const uint64_t rec_cap = std::min<uint64_t>(n_tiles_all * 16, ED_TP_MAX_REC_BYTES / 32);
        // (at least 256 per stripe: a small search's few workgroups each land in one stripe, up to 128 records each)
        const uint64_t rec_share = std::max<uint64_t>((rec_cap + ED_REC_STRIPES - 1) / ED_REC_STRIPES, 256);
        constexpr size_t REC_CTR_BYTES = (size_t)ED_REC_STRIPES * ED_REC_LINE * 4;  // the stripe counters, then records
        Q.rec_cnt = d_rec_cnt;
        // (NMZ_ED_QG_RECOMPUTE=1 skips the records: the recompute path, for tests)
        const char *rc_env = ab_env("NMZ_ED_QG_RECOMPUTE");
        // (the kernels count records with a u32 atomic, up to 128 per tile: a launch that could pass 2^32 of them would
        // wrap the counter, so such searches recompute instead)
        uint4 *d_rec = nullptr;  // one field of bytes, addressed in 16-byte records
        ScratchLayout rec_lay;
        if (!(rc_env && atoi(rc_env) == 1) && n_tiles_all * 128 < (1ULL << 32) &&
            rec_lay.add(&d_rec, (REC_CTR_BYTES + rec_share * ED_REC_STRIPES * 32) / 16).bind(p->tp_rec) == NMZ_OK) {
            Q.recs = d_rec + REC_CTR_BYTES / 16;
            Q.rec_cap = (uint32_t)rec_share;
        }
        // the stripe counters, at the buffer's start
        Q.n_rec = Q.recs ? reinterpret_cast<uint32_t *>(d_rec) : nullptr;
        // (k_tp_scan leaves them at zero; a new allocation -- tp_rec's generation changed, whatever its address -- or
        // an interrupted search clears them here)
        if (Q.n_rec && (p->tp_rec.gen != p->tp_rec_gen || p->tp_dirty)) {
            NMZ_HIP(hipMemsetAsync(Q.n_rec, 0, REC_CTR_BYTES, st));
            p->tp_rec_gen = p->tp_rec.gen;
        }
        rec_total_cap = rec_share * ED_REC_STRIPES;
        Q.N = N;
        Q.k = A.k;
        Q.QB = (N + 63) / 64;
        Q.NCB = (N + 255) / 256;
        Q.shard = A.shard;
        Q.n_shards = A.n_shards;
        Q.w = p->band;
        // entries per DP work item: from the search's entry total (ed_bv_pick_item) unless NMZ_ED_ITEM fixes it
        item = ed_bv_item();
        return NMZ_OK;
    }

    // the offset kernels (tp_offsets) over the latest count pass's counts; verify = a shard's cached sizes to compare with
    int offsets(bool with_rec, const nmz_ed_plan::TpSizes *verify) {
        TpScanArgs S{};
        S.cnt = d_cnt;
        S.n = n_pairs;
        S.agg = d_agg;
        S.poff = d_poff;
        S.ioff = d_ioff;
        S.tot64 = d_tot64;
        S.n_rec = with_rec ? Q.n_rec : nullptr;
        S.rec_out = f + 1;
        S.rec_cnt = d_rec_cnt;
        S.rec_share = Q.rec_cap;
        S.flag = verify ? p->d_tp_mismatch : nullptr;
        S.h_flag = verify ? p->h_tp_flag : nullptr;
        S.seq = p->tp_seq;
        if (verify) {
            // (NMZ_ED_TP_FAKE_MISMATCH=1, a test knob: compare against a wrong total, so the flag path runs)
            const char *fake = ab_env("NMZ_ED_TP_FAKE_MISMATCH");
            S.e_tot = verify->tot64 + ((fake && atoi(fake) == 1) ? 1 : 0);
            S.e_items = verify->items;
            S.e_rec = verify->n_rec;
        }
        const int rc = tp_offsets(S, item, st);
        if (rc == NMZ_OK && S.h_flag) p->tp_seq_sent = S.seq;
        return rc;
    }

    // count pass + scans over a tile list: entry and item totals. With verify (sizes known from an earlier search of
    // this shard) nothing is read back: everything stays on the device
    int count(const uint64_t *tiles, uint64_t n_tiles, const nmz_ed_plan::TpSizes *verify = nullptr) {
        Q.tiles = tiles;
        Q.n_tiles = n_tiles;
        p->tp_dirty = true;  // until the write pass has taken the counts back
        {
            KernelTimer kt(p->ctx, st, "ed_qg_filter");
            NMZ_TRY(ed_qg_filter_launch(Q, true, st));
        }
        // the entry total in 64 bits: the u32 offsets wrap beyond 2^32 entries (about N^2 / 4 for a store of
        // near-duplicates), so they are trusted only once this total is within the limit
        NMZ_TRY(offsets(true, verify));
        if (verify) return NMZ_OK;
        NMZ_HIP(hipMemcpyAsync(&tot64, d_tot64, 8, hipMemcpyDeviceToHost, st));
        NMZ_HIP(hipMemcpyAsync(&tot_items, d_ioff + n_pairs, 4, hipMemcpyDeviceToHost, st));
        if (Q.recs) NMZ_HIP(hipMemcpyAsync(&n_rec, f + 1, 4, hipMemcpyDeviceToHost, st));
        NMZ_HIP(hipStreamSynchronize(st));
        return NMZ_OK;
    }

    // write pass + DP of the tiles the last count pass covered
    int write_dp(uint64_t n_ent, uint32_t n_items) {
        // the u32 scans (entry and item offsets) hold only below 2^32 entries: a batch must never reach it
        NMZ_CHECK(n_ent < (1ULL << 32), "internal: a two-phase batch reaches 2^32 entries");
        ScratchLayout lay;
        NMZ_TRY(lay.add(&Q.ent, n_ent + 1).bind(p->tp_ent));
        Q.ent_cap = n_ent;  // entry writes past the sizes the lists were made for are dropped
        {
            KernelTimer kt(p->ctx, st, "ed_qg_filter");
            if (Q.recs && n_rec <= rec_total_cap) NMZ_TRY(ed_qg_scatter_launch(Q, n_rec, st));
            else NMZ_TRY(ed_qg_filter_launch(Q, false, st));
        }
        p->tp_dirty = false;
        KernelTimer kt(p->ctx, st, "ed_bv_dp");
        return ed_bv_dp_launch(A, d_ioff, d_poff, Q.ent, n_pairs, n_items, item, p->bw, p->cmp, st, f);
    }

    // the DP items of the last count pass again under another item size (the first search of a shard, once its entry
    // total is known)
    int reitem(uint32_t it) {
        item = it;
        NMZ_TRY(offsets(false, nullptr));
        NMZ_HIP(hipMemcpyAsync(&tot_items, d_ioff + n_pairs, 4, hipMemcpyDeviceToHost, st));
        NMZ_HIP(hipStreamSynchronize(st));
        return NMZ_OK;
    }
};

// After a count pass over the whole list tl whose entry total exceeds `limit`: batches of whole query blocks (at least
// one per batch) whose entries fit, each a count pass, scans, the write pass and the DP. Per-block totals come from
// that first count pass, then the lists and counters start over (it listed pairs with an empty trace, and counted).
static int tp_batched(TpSearch &S, const uint64_t *tl, uint64_t n_tiles_all, uint64_t limit, uint64_t *d_knn) {
    nmz_ed_plan *p = S.p;
    hipStream_t st = S.st;
    const uint32_t N = p->n, n_pairs = S.n_pairs;
    std::vector<uint32_t> cnt(n_pairs);
    NMZ_HIP(hipMemcpy(cnt.data(), S.d_cnt, (size_t)n_pairs * 4, hipMemcpyDeviceToHost));
    NMZ_HIP(hipMemsetAsync(S.d_cnt, 0, (n_pairs + 1) * 4, st));  // (no write pass took this count pass's counts)
    std::vector<uint32_t> qbs, grp;
    shard_tiles(S.Q.QB, S.Q.NCB, S.A.shard, S.A.n_shards, qbs, grp, nullptr);
    const size_t ng = grp.size() / 2;
    knn_init_launch(d_knn, (uint64_t)N * S.A.k, st);
    NMZ_HIP(hipMemsetAsync(p->d_counters, 0, ED_CNT_WORDS * 8, st));
    // a query block's entry total (this count pass's per-pair counts)
    auto block_entries = [&](size_t i) {
        uint64_t c = 0;
        for (uint32_t pp = 32 * qbs[i]; pp < std::min(32 * qbs[i] + 32, n_pairs); ++pp) c += cnt[pp];
        return c;
    };
    DevBuf sub;  // the tile list of a batch narrower than one group (uploaded per batch)
    ScopedRelease rel_sub{sub};
    for (size_t b0 = 0; b0 < ng;) {
        uint64_t acc = 0;
        size_t b1 = b0;
        while (b1 < ng) {
            const size_t i1 = b1 + 1 < ng ? grp[2 * (b1 + 1)] : qbs.size();
            uint64_t c = 0;
            for (size_t i = grp[2 * b1]; i < i1; ++i) c += block_entries(i);
            if (acc + c > limit) break;
            acc += c;
            ++b1;
        }
        if (b1 > b0) {  // whole groups: their tiles are one contiguous range of the shard's list
            const uint64_t t0 = grp[2 * b0 + 1], t1 = b1 < ng ? grp[2 * b1 + 1] : n_tiles_all;
            NMZ_TRY(S.count(tl + t0, t1 - t0));
            NMZ_TRY(S.write_dp(S.tot64, S.tot_items));
            b0 = b1;
            continue;
        }
        // one group alone exceeds the limit: its query blocks in sub-batches, each with its own tile list (the
        // group's superblock order, restricted to the sub-batch's blocks); a single block cannot be split further:
        // it runs alone, and fails loudly only at 2^32 entries (64 queries x N candidates: N >= 2^26)
        const size_t i0 = grp[2 * b0], i1 = b0 + 1 < ng ? grp[2 * (b0 + 1)] : qbs.size();
        for (size_t j0 = i0; j0 < i1;) {
            uint64_t a = 0;
            size_t j1 = j0;
            while (j1 < i1 && (j1 == j0 || a + block_entries(j1) <= limit)) a += block_entries(j1++);
            // (a block alone may pass the batching limit; it must stay below the u32 scans' 2^32)
            NMZ_CHECK(a < (1ULL << 32), "one query block's candidate entries reach 2^32 (too many traces)");
            std::vector<uint64_t> tiles;
            superblock_tiles(qbs, j0, j1, S.Q.NCB, &tiles);
            uint64_t *d_tiles;
            ScratchLayout lay;
            NMZ_TRY(lay.add(&d_tiles, tiles.size() + 1).bind(sub));
            NMZ_HIP(hipStreamSynchronize(st));  // the previous sub-batch's kernels have read the list
            if (!tiles.empty())  // synchronous: the list is pageable and reused at once
                NMZ_HIP(hipMemcpy(d_tiles, tiles.data(), tiles.size() * sizeof(uint64_t), hipMemcpyHostToDevice));
            NMZ_TRY(S.count(d_tiles, tiles.size()));
            NMZ_TRY(S.write_dp(S.tot64, S.tot_items));
            j0 = j1;
        }
        b0 = b0 + 1;
    }
    return NMZ_OK;
}

// The shard's tiles in query-block order; the count pass sizes the entry lists. Entry lists beyond
// ed_tp_max_entries() are split (tp_batched). Every shard of a search therefore covers exactly its own query
// blocks, whatever its entry total (a single-kernel fallback per shard deals pairs by a different rule, and shards
// that chose differently would drop or double pairs). Returns 1 only when the plan cannot take the two-phase search
// at all (N >= 2^30: entries carry j in 30 bits), the same on every shard.
int ed_bv_two_phase(nmz_ed_plan *p, hipStream_t st, EdBvArgs &A, uint64_t *d_knn) {
    const uint32_t N = p->n;
    if (N >= (1u << 30)) return 1;
    // this shard's tiles (qb << 32 | cb), built and uploaded once per (shard, n_shards)
    const uint64_t key = ((uint64_t)A.shard << 32) | A.n_shards;
    DevBuf &tl = p->tile_list[key];
    if (!p->tile_count.count(key)) {
        std::vector<uint32_t> qbs, grp;
        std::vector<uint64_t> tiles;
        shard_tiles((N + 63) / 64, (N + 255) / 256, A.shard, A.n_shards, qbs, grp, &tiles);
        uint64_t *d_tiles;
        ScratchLayout lay;
        NMZ_TRY(lay.add(&d_tiles, tiles.size() + 1).bind(tl));
        if (!tiles.empty())  // synchronous: the list is pageable
            NMZ_HIP(hipMemcpy(d_tiles, tiles.data(), tiles.size() * sizeof(uint64_t), hipMemcpyHostToDevice));
        p->tile_count[key] = tiles.size();
    }
    const uint64_t n_tiles_all = p->tile_count[key];
    TpSearch S{p, st, A};
    NMZ_TRY(S.setup(n_tiles_all));
    const uint64_t limit = std::min<uint64_t>(ed_tp_max_entries(), 0xFFFFFFFFull);
    // The sizes the host needs before the write pass and the DP (entry total, work items, survivor records) are
    // fixed by the plan and the shard: the first search of a shard reads them back (one synchronisation), later
    // searches enqueue every kernel with those sizes and no host round trip; a one-thread kernel compares them with
    // this search's own totals and flags a difference. None can occur (the plan is immutable and the filter
    // deterministic), but if one did, the flagged search's write pass and DP skip (no write past lists sized for the
    // cached totals, no DP over offsets that disagree with them) and the shard's next search, or the next
    // synchronous call, reports it and drops the cache (ed_tp_flag_check)
    auto cached = p->tp_sizes.find(key);
    if (cached != p->tp_sizes.end() && S.Q.recs && cached->second.tot64 <= limit) {
        const nmz_ed_plan::TpSizes &z = cached->second;
        S.item = z.item;
        NMZ_TRY(ed_tp_flag_host(p));
        ++p->tp_seq;  // this search's number: its scan publishes it with the flag
        NMZ_TRY(S.count(tl.as<uint64_t>(), n_tiles_all, &z));
        S.n_rec = z.n_rec;
        NMZ_TRY(S.write_dp(z.tot64, z.items));
        p->tp_flag_armed = true;  // the search's scan publishes {tp_seq, flag} to h_tp_flag
        return NMZ_OK;
    }
    // uncached: the count pass's totals come back to the host
    NMZ_TRY(S.count(tl.as<uint64_t>(), n_tiles_all));
    if (S.tot64 <= limit) {
        const uint32_t it = ed_bv_pick_item(S.tot64);
        if (it != S.item) NMZ_TRY(S.reitem(it));
        if (S.Q.recs && S.n_rec <= S.rec_total_cap)
            p->tp_sizes[key] = nmz_ed_plan::TpSizes{S.tot64, S.tot_items, S.n_rec, S.item};
        return S.write_dp(S.tot64, S.tot_items);
    }
    return tp_batched(S, tl.as<uint64_t>(), n_tiles_all, limit, d_knn);
}

}  // namespace nmz

using namespace nmz;

extern "C" {

int nmz_debug_tp_offsets(nmz_ctx *ctx, const uint32_t *d_cnt, uint32_t n, uint32_t item, uint32_t *d_poff,
                         uint32_t *d_ioff, uint64_t *d_tot, void *stream) {
    NMZ_CHECK(ctx != nullptr && d_cnt != nullptr && d_poff != nullptr && d_ioff != nullptr && d_tot != nullptr,
              "NULL argument");
    NMZ_CHECK(n > 0 && n < (1u << 30), "n out of range");
    NMZ_CHECK(item > 0 && (item & (item - 1)) == 0, "item must be a power of two");
    NMZ_CHECK(((uintptr_t)d_cnt & 15) == 0, "d_cnt must be 16-byte aligned (the scan loads uint4)");
    CtxGuard g(ctx);
    NMZ_TRY(g.rc);
    hipStream_t st = stream ? (hipStream_t)stream : ctx->stream;
    DevBuf agg;
    ScopedRelease rel{agg};
    NMZ_TRY(agg.ensure(2 * TP_MAX_BLOCKS * 8));
    TpScanArgs S{};
    S.cnt = d_cnt;
    S.n = n;
    S.agg = agg.as<uint64_t>();
    S.poff = d_poff;
    S.ioff = d_ioff;
    S.tot64 = d_tot;
    NMZ_TRY(tp_offsets(S, item, st));
    NMZ_HIP(hipStreamSynchronize(st));
    return NMZ_OK;
}

}  // extern "C"
