// K3 plans (ed_plan.h nmz_ed_plan): the remap of the symbols to dense 16-bit ids (exact: equality preserved) and the
// device layout of each plan kind -- bit-parallel (ed_bv.hip), wide (ed_wide.hip), tile (k_ed_tile) and generic.
// Large stores build the first two on the device (sort/unique, then a remap kernel), the others remap through a hash
// map on the host; both builders of a kind share its shape, stream layout and storage.
#include <algorithm>

#include "ed_plan.h"

namespace nmz {

// stored streams of the bit-parallel plan from device symbols: one block per trace, each symbol's dense id is its
// rank among the sorted distinct symbols (binary search), written as its Peq row's byte offset (id * ndw * 8), or
// as the id itself for compact tables (row_bytes = 1)
__global__ __launch_bounds__(256) void k_ed_bv_remap(const uint64_t *__restrict__ off, const uint64_t *__restrict__ sym,
                                                     const uint64_t *__restrict__ uniq, uint32_t n_uniq,
                                                     const uint64_t *__restrict__ soff, uint32_t row_bytes,
                                                     uint16_t *__restrict__ bs) {
    const uint32_t i = blockIdx.x;
    const uint64_t b = off[i], n = off[i + 1] - b, so = soff[i];
    for (uint64_t t = threadIdx.x; t < n; t += 256) {
        const uint64_t x = sym[b + t];
        uint32_t lo = 0, hi = n_uniq;  // first index with uniq[idx] >= x (x is present)
        while (lo < hi) {
            const uint32_t mid = (lo + hi) >> 1;
            if (uniq[mid] < x) lo = mid + 1; else hi = mid;
        }
        bs[so + t] = (uint16_t)(lo * row_bytes);
    }
}

// per trace: the number of distinct stream values (symbol ids < n_ids), one workgroup per trace with an LDS bitmap
__global__ __launch_bounds__(256) void k_trace_distinct(const uint16_t *__restrict__ bs, const uint64_t *__restrict__ soff,
                                                        const uint32_t *__restrict__ len, uint32_t n_ids,
                                                        uint32_t *__restrict__ out) {
    extern __shared__ uint32_t bits[];
    const uint32_t i = blockIdx.x, nw = (n_ids + 31) / 32;
    for (uint32_t t = threadIdx.x; t < nw; t += 256) bits[t] = 0;
    __syncthreads();
    const uint16_t *a = bs + soff[i];
    for (uint32_t t = threadIdx.x; t < len[i]; t += 256) atomicOr(&bits[a[t] >> 5], 1u << (a[t] & 31));
    __syncthreads();
    uint32_t c = 0;
    for (uint32_t t = threadIdx.x; t < nw; t += 256) c += __builtin_popcount(bits[t]);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) c += __shfl_xor(c, off, 64);
    __shared__ uint32_t part[4];
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) out[i] = part[0] + part[1] + part[2] + part[3];
}

// wide-band plan streams from device symbols: dense id (rank among the sorted distinct symbols) per position, in
// CSR order (qsym), and the id's Peq row byte offset per position of each trace's padded row stream (rowb)
__global__ __launch_bounds__(256) void k_ed_wide_remap(const uint64_t *__restrict__ off, const uint64_t *__restrict__ sym,
                                                       const uint64_t *__restrict__ uniq, uint32_t n_uniq,
                                                       const uint64_t *__restrict__ roff, uint32_t row_bytes,
                                                       uint16_t *__restrict__ qsym, uint32_t *__restrict__ rowb) {
    const uint32_t i = blockIdx.x;
    const uint64_t b = off[i], n = off[i + 1] - b, ro = roff[i];
    for (uint64_t t = threadIdx.x; t < n; t += 256) {
        const uint64_t x = sym[b + t];
        uint32_t lo = 0, hi = n_uniq;  // first index with uniq[idx] >= x (x is present)
        while (lo < hi) {
            const uint32_t mid = (lo + hi) >> 1;
            if (uniq[mid] < x) lo = mid + 1; else hi = mid;
        }
        qsym[b + t] = (uint16_t)lo;
        rowb[ro + t] = lo * row_bytes;
    }
}

// LDS extras of the pool kernels beyond the tables: counters, two q-gram profiles, a pool's survivor list
static size_t bv_pool_extras(uint32_t pool) { return 16 + 2 * ED_QG_DW * 4 + ((size_t)pool * 2 + 15) / 16 * 16; }

bool bv_compact_layout(uint32_t n_ids, uint32_t R, uint32_t ndw, size_t extras, size_t limit, uint32_t &lds_dw,
                       uint32_t &rmap_dw, uint32_t &claim_dw) {
    const uint64_t rows_bytes = (uint64_t)(R + 1) * ndw * 8;
    const uint64_t peq_dw = (rows_bytes / 4 + 3) / 4 * 4;
    const uint64_t map_dw = ((n_ids + 2) / 2 + 3) / 4 * 4;
    const uint64_t clm_dw = ((n_ids + 32) / 32 + 3) / 4 * 4;
    const uint64_t total = peq_dw + map_dw + clm_dw;
    if (rows_bytes > 65535 || total * 4 + extras > limit) return false;
    lds_dw = (uint32_t)total;
    rmap_dw = (uint32_t)peq_dw;
    claim_dw = (uint32_t)(peq_dw + map_dw);
    return true;
}

// stores of at least this many symbols are remapped on the device; smaller stores keep the host remap
constexpr uint64_t ED_DEVICE_REMAP_MIN = 1ULL << 20;

// A/B knobs set to 0: NMZ_ED_QGRAM turns off the q-gram lower-bound filter of the bit-parallel kernels (ed_bv.hip);
// NMZ_ED_TWO_PHASE keeps the single-kernel search with its in-workgroup pre-filter instead of the two-phase search
// (filter tiles, then DP work items) that the filter otherwise brings
static bool knob_off(const char *name) {
    const char *e = ab_env(name);
    return e && atoi(e) == 0;
}

// queries per block row of the bit-parallel search (NMZ_ED_RW overrides the multiple of 64 for A/B runs)
static uint32_t ed_bv_row_queries() {
    static const uint32_t rq = [] {
        const char *e = ab_env("NMZ_ED_RW");
        const int v = e ? atoi(e) : (int)ED_BV_RW;
        return 64u * (uint32_t)((v >= 1 && v <= 32) ? v : (int)ED_BV_RW);
    }();
    return rq;
}

void ed_plan_release(nmz_ed_plan *p) {
    if (!p) return;
    p->mem.release();
    p->tp_mem.release();
    p->tp_ent.release();
    p->tp_rec.release();
    for (auto &kv : p->tile_list) kv.second.release();
    ed_tp_flag_release(p);
    delete p;
}

// ---- bit-parallel plan ----
// Shape: the kernels' band and row stride, the pool, direct or compact tables, the block rows. Direct tables (every
// symbol of the store has a row) when they fit beside the pool kernels' extras, else compact tables (per-query Peq
// rows for the symbols of one query pair only; bv_plan_compact sizes them from the traces' distinct counts).
// Candidates per workgroup: a larger pool amortises the Peq build and evens out the lanes' refill tail, a smaller
// one keeps enough workgroups for small N (configs[2]-shaped traces, 1 MI355X: N = 100k: 1024 -> 1.78 s, 4096 ->
// 1.64 s, 8192 -> 1.65 s; N = 8192: 1024 -> 14.5 ms, 4096 -> 19.6 ms)
static void bv_plan_shape(nmz_ed_plan *p, uint32_t n_sym, bool compact_opt) {
    const uint32_t N = p->n;
    p->bw = ed_bv_template(p->band);
    const uint32_t KF = (2 * p->bw + 31) / 32;
    p->ndw = ((p->maxlen + 31) / 32 + KF + 2) | 1;  // odd row stride: rows of distinct symbols start on distinct bank pairs
    p->row_bytes = p->ndw * 8;
    p->pool = N >= 24576 ? 4 * ED_BV_POOL : (N >= 12288 ? 2 * ED_BV_POOL : ED_BV_POOL);
    if (const char *e = ab_env("NMZ_ED_POOL")) {
        const uint32_t v = (uint32_t)atoi(e);
        if (v >= 256 && v % 256 == 0 && v <= 16384) p->pool = v;
    }
    const uint64_t direct_bytes = (((uint64_t)(n_sym + 1) * p->ndw * 8 + 15) / 16) * 16;
    p->cmp = direct_bytes + bv_pool_extras(p->pool) > 65536 || compact_opt;
    if (p->cmp) p->pool = std::min(p->pool, ED_BV_POOL);  // the single kernel's survivor list leaves room for rows
    p->lds_dw = (uint32_t)(direct_bytes / 4);
    p->rq = ed_bv_row_queries();
    p->G = (N + p->rq - 1) / p->rq;
    p->n_sym = n_sym;
}

// compact tables from the traces' distinct symbol counts d[N]: false when even a query pair's own symbols do not fit
static bool bv_plan_compact(nmz_ed_plan *p, const std::vector<uint32_t> &d) {
    uint32_t r = 0;  // the rows one workgroup's tables need: the largest d(2p) + d(2p + 1) over the query pairs
    for (size_t i = 0; i < d.size(); i += 2) r = std::max(r, d[i] + (i + 1 < d.size() ? d[i + 1] : 0u));
    return bv_compact_layout(p->n_sym, r, p->ndw, bv_pool_extras(p->pool), 65536, p->lds_dw,
                             p->rmap_dw, p->claim_dw);
}

// Stream layout: each trace's stream padded to whole 32-blocks + 1 spare; per block row, its chunks of `pool`
// candidates
struct BvStreams {
    std::vector<uint32_t> len;
    std::vector<uint64_t> soff, chunk_start;
    uint64_t bs_n;       // stream elements, + 2 spare blocks at the end
    uint16_t zero_row;   // padding: the zero row's offset (direct), or the id n_sym, which never gets a row (compact)
};

static BvStreams bv_plan_streams(nmz_ed_plan *p, const uint64_t *off) {
    const uint32_t N = p->n, G = p->G;
    BvStreams s;
    s.len.assign(N + 1, 0);
    s.soff.assign(N + 1, 0);
    s.chunk_start.assign(G + 1, 0);
    for (uint32_t i = 0; i < N; ++i) {
        s.len[i] = (uint32_t)(off[i + 1] - off[i]);
        s.soff[i + 1] = s.soff[i] + ((uint64_t)(s.len[i] + 31) / 32 + 1) * 32;
    }
    for (uint32_t b = 0; b < G; ++b)
        s.chunk_start[b + 1] = s.chunk_start[b] + (N - p->rq * b + p->pool - 1) / p->pool;
    p->n_chunks = s.chunk_start[G];
    s.bs_n = s.soff[N] + 64;
    s.zero_row = (uint16_t)(p->cmp ? p->n_sym : p->n_sym * p->ndw * 8);
    return s;
}

// Storage: the plan's memory, its carve, the uploads of the layout (s stays alive until the stream is synchronised)
// and the counters' first clear. d_bsym is left for the builder to fill.
static int bv_plan_storage(nmz_ed_plan *p, const BvStreams &s, const uint64_t *off, hipStream_t st) {
    const uint32_t N = p->n, G = p->G;
    ScratchLayout lay;
    lay.add(&p->d_counters, ED_CNT_WORDS).add(&p->d_prof, (uint64_t)N * ED_QG_DW).add(&p->d_bsym, s.bs_n);
    lay.add(&p->d_soff, N + 1).add(&p->d_qoff, N + 1).add(&p->d_chunk_start, G + 1).add(&p->d_len, N + 1);
    NMZ_TRY(lay.bind(p->mem));
    NMZ_TRY(copy_h2d(p->d_soff, s.soff.data(), (size_t)N + 1, st));
    NMZ_TRY(copy_h2d(p->d_qoff, off, (size_t)N + 1, st));
    NMZ_TRY(copy_h2d(p->d_chunk_start, s.chunk_start.data(), (size_t)G + 1, st));
    NMZ_TRY(copy_h2d(p->d_len, s.len.data(), (size_t)N + 1, st));
    NMZ_HIP(hipMemsetAsync(p->d_counters, 0, ED_CNT_WORDS * 8, st));
    return NMZ_OK;
}

// the device builders' scratch: the store's symbols (uploaded from sym unless d_sym_in has them:
// nmz_ed_plan_create_dev), its sorted distinct symbols, n_off offset arrays of N + 1
struct DeviceSymbols {
    const uint64_t *d_sym;
    uint64_t *d_uniq, *d_off[2];
    uint64_t n_uniq = 0;
};

static int device_symbols(DevBuf &tmp, const uint64_t *off, const uint64_t *sym, const uint64_t *d_sym_in, uint32_t N,
                          uint32_t n_off, hipStream_t st, DeviceSymbols &D) {
    const uint64_t total = off[N];
    NMZ_CHECK(total == 0 || sym || d_sym_in, "sym is NULL");
    uint64_t *d_up = nullptr;
    ScratchLayout lay;
    if (!d_sym_in) lay.add(&d_up, total);
    lay.add(&D.d_uniq, MAX_FAST_SYMBOLS + 1);
    for (uint32_t i = 0; i < n_off; ++i) lay.add(&D.d_off[i], N + 1);
    NMZ_TRY(lay.bind(tmp));
    NMZ_TRY(copy_h2d(d_up, sym, d_sym_in ? 0 : total, st));
    D.d_sym = d_sym_in ? d_sym_in : d_up;
    NMZ_TRY(copy_h2d(D.d_off[0], off, (size_t)N + 1, st));
    return device_unique_u64(D.d_sym, total, D.d_uniq, MAX_FAST_SYMBOLS, &D.n_uniq, st);
}

// the dictionary for single queries (nmz_ed_plan_query_knn): symbol -> rank; synchronises st
static int device_dict(nmz_ed_plan *p, const DeviceSymbols &D, hipStream_t st) {
    std::vector<uint64_t> uniq(D.n_uniq);
    if (D.n_uniq) NMZ_HIP(hipMemcpyAsync(uniq.data(), D.d_uniq, D.n_uniq * 8, hipMemcpyDeviceToHost, st));
    NMZ_HIP(hipStreamSynchronize(st));  // the builders' host vectors are pageable; their scratch goes back
    p->dict.reserve(D.n_uniq * 2);
    for (uint64_t i = 0; i < D.n_uniq; ++i) p->dict.emplace(uniq[i], (uint32_t)i);
    return NMZ_OK;
}

// The bit-parallel plan built on the device: upload the symbols, sort/unique them (dense ids = ranks), write the
// candidate streams with a binary search per symbol. Returns 1 (not applicable: the alphabet does not fit the
// bit-parallel LDS tables) so the caller falls back to the host build and the other kernels.
static int ed_plan_build_bv_device(nmz_ed_plan *p, const uint64_t *off, const uint64_t *sym, const uint64_t *d_sym_in,
                                   bool compact_opt) {
    hipStream_t st = p->ctx->stream;
    const uint32_t N = p->n;
    DevBuf tmp;
    ScopedRelease release_tmp{tmp};
    DeviceSymbols D;
    NMZ_TRY(device_symbols(tmp, off, sym, d_sym_in, N, 1, st, D));
    if (D.n_uniq >= MAX_FAST_SYMBOLS) return 1;
    bv_plan_shape(p, (uint32_t)D.n_uniq, compact_opt);
    const uint32_t n_sym = p->n_sym;
    const BvStreams s = bv_plan_streams(p, off);
    NMZ_TRY(bv_plan_storage(p, s, off, st));
    NMZ_HIP(hipMemsetD16Async((hipDeviceptr_t)p->d_bsym, s.zero_row, s.bs_n, st));
    hipLaunchKernelGGL(k_ed_bv_remap, dim3(N), dim3(256), 0, st, D.d_off[0], D.d_sym, D.d_uniq, n_sym, p->d_soff,
                       p->cmp ? 1u : p->ndw * 8, p->d_bsym);
    NMZ_HIP(hipGetLastError());
    if (p->cmp) {  // the traces' distinct counts size the per-workgroup rows
        DevBuf dbuf;
        ScopedRelease rel{dbuf};
        uint32_t *d_distinct;
        ScratchLayout dlay;
        NMZ_TRY(dlay.add(&d_distinct, N + 1).bind(dbuf));
        hipLaunchKernelGGL(k_trace_distinct, dim3(N), dim3(256), ((n_sym + 32) / 32) * 4, st, p->d_bsym, p->d_soff,
                           p->d_len, n_sym + 1, d_distinct);
        NMZ_HIP(hipGetLastError());
        std::vector<uint32_t> d(N);
        NMZ_TRY(copy_d2h(d.data(), d_distinct, N, st));
        NMZ_HIP(hipStreamSynchronize(st));
        if (!bv_plan_compact(p, d)) return 1;  // the host build's other kernels
    }
    NMZ_TRY(ed_qgram_profiles(p->d_bsym, p->d_soff, p->d_len, N, p->d_prof, st));
    NMZ_TRY(device_dict(p, D, st));
    p->bv = p->fast = true;
    return NMZ_OK;
}

// The bit-parallel plan from the host remap (ids: dense id per symbol, CSR order). Returns 1 (the compact tables do
// not fit) before it allocates anything.
static int ed_plan_build_bv_host(nmz_ed_plan *p, const uint64_t *off, const std::vector<uint16_t> &ids,
                                 std::unordered_map<uint64_t, uint32_t> &dict, bool compact_opt) {
    hipStream_t st = p->ctx->stream;
    const uint32_t N = p->n;
    bv_plan_shape(p, (uint32_t)dict.size(), compact_opt);
    if (p->cmp) {
        std::vector<uint32_t> d(N, 0), stamp(p->n_sym + 1, UINT32_MAX);
        for (uint32_t i = 0; i < N; ++i)
            for (uint64_t t = off[i]; t < off[i + 1]; ++t)
                if (stamp[ids[t]] != i) {
                    stamp[ids[t]] = i;
                    ++d[i];
                }
        if (!bv_plan_compact(p, d)) return 1;
    }
    const BvStreams s = bv_plan_streams(p, off);
    std::vector<uint16_t> bs(s.bs_n, s.zero_row);
    for (uint32_t i = 0; i < N; ++i)
        for (uint32_t t = 0; t < s.len[i]; ++t)
            bs[s.soff[i] + t] = (uint16_t)(p->cmp ? ids[off[i] + t] : ids[off[i] + t] * p->ndw * 8);
    NMZ_TRY(bv_plan_storage(p, s, off, st));
    NMZ_HIP(hipMemcpyAsync(p->d_bsym, bs.data(), bs.size() * 2, hipMemcpyHostToDevice, st));
    NMZ_TRY(ed_qgram_profiles(p->d_bsym, p->d_soff, p->d_len, N, p->d_prof, st));
    NMZ_HIP(hipStreamSynchronize(st));
    p->dict = std::move(dict);
    p->bv = p->fast = true;
    return NMZ_OK;
}

// ---- wide plan ----
// Shape: the kernel's W, the dwords per Peq row; false when the alphabet's tables are too large (p->ww stays: the
// fingerprint of the generic plan that follows has always carried it)
static bool wide_plan_shape(nmz_ed_plan *p, uint32_t n_ids) {
    const uint32_t n_sym = std::max(n_ids, 1u);
    p->ww = ed_wide_template(p->band);
    const uint32_t ndw = ed_wide_ndw(p->ww, p->maxlen);
    const uint64_t peq_bytes = (uint64_t)p->n * n_sym * ndw * 4;
    // one query's table must be addressable by a 32-bit buffer offset
    if (peq_bytes > (16ULL << 30) || (uint64_t)n_sym * ndw * 4 >= (1ULL << 31)) return false;
    p->ndw = ndw;
    p->n_sym = n_sym;
    return true;
}

// per-position Peq row byte offsets, each trace padded to whole 32-column blocks + 2 spare blocks: the traces' starts
static std::vector<uint64_t> wide_plan_roff(const uint64_t *off, uint32_t N) {
    std::vector<uint64_t> roff(N + 1, 0);
    for (uint32_t i = 0; i < N; ++i) roff[i + 1] = roff[i] + ((off[i + 1] - off[i] + 31) / 32 + 2) * 32;
    return roff;
}

// Storage: the plan's memory, its carve, the offsets' uploads (roff stays alive until the stream is synchronised)
// and zeroed dense ids. d_qsym's ids and d_rowb (roff[N] + 1 entries) are left for the builder to fill.
static int wide_plan_storage(nmz_ed_plan *p, const uint64_t *off, const std::vector<uint64_t> &roff, hipStream_t st) {
    const uint32_t N = p->n;
    const uint64_t total = p->total, nrow = roff[N] + 1;
    ScratchLayout lay;
    lay.add(&p->d_qsym, total + 64).add(&p->d_qoff, N + 1).add(&p->d_peq, (uint64_t)N * p->n_sym * p->ndw);
    lay.add(&p->d_rowb, nrow).add(&p->d_rowb_off, N + 1);
    NMZ_TRY(lay.bind(p->mem));
    NMZ_TRY(copy_h2d(p->d_qoff, off, (size_t)N + 1, st));
    NMZ_TRY(copy_h2d(p->d_rowb_off, roff.data(), (size_t)N + 1, st));
    NMZ_HIP(hipMemsetAsync(p->d_qsym, 0, (total + 64) * 2, st));
    return NMZ_OK;
}

// The wide-band plan built on the device (the host build remaps every symbol through a hash map: ~100 ms for
// configs[4]'s 1.7e7 symbols): distinct symbols from the device sort, then one remap kernel. Returns 1 (not
// applicable: alphabet or Peq tables too large) so the caller takes the host build.
static int ed_plan_build_wide_device(nmz_ed_plan *p, const uint64_t *off, const uint64_t *sym,
                                     const uint64_t *d_sym_in) {
    hipStream_t st = p->ctx->stream;
    const uint32_t N = p->n;
    DevBuf tmp;
    ScopedRelease release_tmp{tmp};
    DeviceSymbols D;
    NMZ_TRY(device_symbols(tmp, off, sym, d_sym_in, N, 2, st, D));
    if (D.n_uniq >= MAX_FAST_SYMBOLS || !wide_plan_shape(p, (uint32_t)D.n_uniq)) return 1;
    const std::vector<uint64_t> roff = wide_plan_roff(off, N);
    NMZ_TRY(wide_plan_storage(p, off, roff, st));
    NMZ_TRY(copy_h2d(D.d_off[1], roff.data(), (size_t)N + 1, st));
    NMZ_HIP(hipMemsetAsync(p->d_rowb, 0, (roff[N] + 1) * 4, st));
    if (N) {
        hipLaunchKernelGGL(k_ed_wide_remap, dim3(N), dim3(256), 0, st, D.d_off[0], D.d_sym, D.d_uniq,
                           (uint32_t)D.n_uniq, D.d_off[1], p->ndw * 4, p->d_qsym, p->d_rowb);
        NMZ_HIP(hipGetLastError());
    }
    NMZ_TRY(ed_wide_build_peq(p->d_qsym, p->d_qoff, N, p->n_sym, p->ndw, p->ww, p->d_peq, st));
    NMZ_TRY(device_dict(p, D, st));
    p->wide = p->fast = true;
    return NMZ_OK;
}

// The wide plan from the host remap. Returns 1 (tables too large) before it allocates anything.
static int ed_plan_build_wide_host(nmz_ed_plan *p, const uint64_t *off, const std::vector<uint16_t> &ids,
                                   std::unordered_map<uint64_t, uint32_t> &dict) {
    hipStream_t st = p->ctx->stream;
    const uint32_t N = p->n;
    if (!wide_plan_shape(p, (uint32_t)dict.size())) return 1;
    const std::vector<uint64_t> roff = wide_plan_roff(off, N);
    std::vector<uint32_t> rowb(roff[N] + 1, 0);
    for (uint32_t i = 0; i < N; ++i)
        for (uint64_t t = off[i]; t < off[i + 1]; ++t) rowb[roff[i] + (t - off[i])] = ids[t] * p->ndw * 4;
    NMZ_TRY(wide_plan_storage(p, off, roff, st));
    NMZ_TRY(copy_h2d(p->d_rowb, rowb.data(), rowb.size(), st));
    NMZ_TRY(copy_h2d(p->d_qsym, ids.data(), p->total, st));
    NMZ_TRY(ed_wide_build_peq(p->d_qsym, p->d_qoff, N, p->n_sym, p->ndw, p->ww, p->d_peq, st));
    NMZ_HIP(hipStreamSynchronize(st));
    p->dict = std::move(dict);
    p->wide = p->fast = true;
    return NMZ_OK;
}

// ---- tile and generic plans ----
// k_ed_tile's plan: the dense ids in CSR order (queries) and lane-interleaved per group of 64 traces (candidates)
static int ed_plan_build_tile(nmz_ed_plan *p, const uint64_t *off, const std::vector<uint16_t> &ids,
                              std::unordered_map<uint64_t, uint32_t> &dict) {
    hipStream_t st = p->ctx->stream;
    const uint32_t N = p->n, G = (N + 63) / 64;
    const uint64_t total = p->total;
    p->G = G;
    std::vector<uint32_t> gmax(G + 1, 0), len(N + 1, 0);
    std::vector<uint64_t> coff(G + 1, 0);
    for (uint32_t i = 0; i < N; ++i) {
        len[i] = (uint32_t)(off[i + 1] - off[i]);
        gmax[i / 64] = std::max(gmax[i / 64], len[i]);
    }
    for (uint32_t g = 0; g < G; ++g) coff[g + 1] = coff[g] + (uint64_t)gmax[g] * 64;
    std::vector<uint16_t> cs(coff[G] + 1, CAND_PAD);
    for (uint32_t i = 0; i < N; ++i) {
        const uint64_t base = coff[i / 64] + (i % 64);
        for (uint32_t t = 0; t < len[i]; ++t) cs[base + (uint64_t)t * 64] = ids[off[i] + t];
    }
    ScratchLayout lay;
    lay.add(&p->d_qsym, total + 1).add(&p->d_csym, cs.size()).add(&p->d_qoff, N + 1).add(&p->d_coff, G + 1);
    lay.add(&p->d_gmax, G + 1).add(&p->d_len, N + 1);
    NMZ_TRY(lay.bind(p->mem));
    NMZ_TRY(copy_h2d(p->d_qsym, ids.data(), total, st));
    NMZ_TRY(copy_h2d(p->d_csym, cs.data(), cs.size(), st));
    NMZ_TRY(copy_h2d(p->d_qoff, off, (size_t)N + 1, st));
    NMZ_TRY(copy_h2d(p->d_coff, coff.data(), (size_t)G + 1, st));
    NMZ_TRY(copy_h2d(p->d_gmax, gmax.data(), (size_t)G + 1, st));
    NMZ_TRY(copy_h2d(p->d_len, len.data(), (size_t)N + 1, st));
    NMZ_HIP(hipStreamSynchronize(st));
    p->dict = std::move(dict);
    p->tile = p->fast = true;
    return NMZ_OK;
}

// the generic plan: offsets and u64 symbols as they came
static int ed_plan_build_generic(nmz_ed_plan *p, const uint64_t *off, const uint64_t *sym) {
    hipStream_t st = p->ctx->stream;
    const uint32_t N = p->n;
    ScratchLayout lay;
    NMZ_TRY(lay.add(&p->d_off64, N + 1).add(&p->d_sym64, p->total + 1).bind(p->mem));
    NMZ_TRY(copy_h2d(p->d_off64, off, (size_t)N + 1, st));
    NMZ_TRY(copy_h2d(p->d_sym64, sym, p->total, st));
    NMZ_HIP(hipStreamSynchronize(st));
    return NMZ_OK;
}

// dense symbol ids on the host (exact remap: a == b <=> id(a) == id(b)); false when the alphabet exceeds
// MAX_FAST_SYMBOLS
static bool host_remap(const uint64_t *sym, uint64_t total, std::unordered_map<uint64_t, uint32_t> &dict,
                       std::vector<uint16_t> &ids) {
    dict.reserve(1024);
    ids.resize(total);
    for (uint64_t t = 0; t < total; ++t) {
        auto it = dict.find(sym[t]);
        uint32_t id;
        if (it == dict.end()) {
            id = (uint32_t)dict.size();
            if (id >= MAX_FAST_SYMBOLS) return false;
            dict.emplace(sym[t], id);
        } else {
            id = it->second;
        }
        ids[t] = (uint16_t)id;
    }
    return true;
}

int ed_plan_build(nmz_ctx *ctx, const uint64_t *off, const uint64_t *sym, uint32_t N, uint32_t band,
                  nmz_ed_plan **out, const uint64_t *d_sym, uint32_t opts) {
    NMZ_CHECK(ctx && out, "NULL argument");
    NMZ_CHECK(N == 0 || off, "off is NULL");
    NMZ_CHECK((opts & ~(uint32_t)(NMZ_ED_OPT_SINGLE_KERNEL | NMZ_ED_OPT_NO_QGRAM | NMZ_ED_OPT_COMPACT |
                                  NMZ_ED_OPT_HOST_BUILD)) == 0, "unknown plan option bits");
    // the A/B environment knobs (NMZ_AB=1 only) add to the options
    if (knob_off("NMZ_ED_TWO_PHASE")) opts |= NMZ_ED_OPT_SINGLE_KERNEL;
    if (knob_off("NMZ_ED_QGRAM")) opts |= NMZ_ED_OPT_NO_QGRAM;
    if (ab_env("NMZ_ED_COMPACT")) opts |= NMZ_ED_OPT_COMPACT;
    if (ab_env("NMZ_ED_HOST_REMAP")) opts |= NMZ_ED_OPT_HOST_BUILD;
    const bool compact_opt = (opts & NMZ_ED_OPT_COMPACT) != 0, host_build = (opts & NMZ_ED_OPT_HOST_BUILD) != 0;
    *out = nullptr;
    // what every kind of plan starts from (a builder that turns out not applicable leaves the plan at this again)
    nmz_ed_plan blank;
    blank.qgram = !(opts & NMZ_ED_OPT_NO_QGRAM);
    blank.two_phase = !(opts & NMZ_ED_OPT_SINGLE_KERNEL);
    blank.opts = opts;
    blank.ctx = ctx;
    blank.n = N;
    blank.band = band;
    const uint64_t total = blank.total = N ? off[N] : 0;
    uint64_t h = 0xcbf29ce484222325ull;  // FNV-1a over the offsets: the store's shape, for the fingerprint
    for (uint32_t i = 0; i <= N; ++i) h = (h ^ off[i]) * 0x100000001b3ull;
    blank.off_hash = h;
    for (uint32_t i = 0; i < N; ++i) blank.maxlen = std::max<uint32_t>(blank.maxlen, (uint32_t)(off[i + 1] - off[i]));
    const uint32_t maxlen = blank.maxlen;
    EdPlanPtr p(new nmz_ed_plan(blank));
    const bool want_wide = ed_wide_supported(band);
    const bool want_bv = ed_bv_supported(band) && maxlen + ed_bv_template(band) < MAX_FAST_LEN;
    const bool tile_band = band == 8 || band == 16 || band == 32;  // k_ed_tile computes exactly its W
    // large stores: the device builders (1: not applicable, the host build below and perhaps the other kernels)
    int rc = 1;
    if (total >= ED_DEVICE_REMAP_MIN && !host_build) {
        if (want_bv && total < (1ULL << 31)) {
            rc = ed_plan_build_bv_device(p.get(), off, sym, d_sym, compact_opt);
            if (rc == 1) p.reset(new nmz_ed_plan(blank));
        }
        if (rc == 1 && want_wide) {
            rc = ed_plan_build_wide_device(p.get(), off, sym, d_sym);
            if (rc == 1) p.reset(new nmz_ed_plan(blank));
        }
    }
    if (rc == 1) {
        std::vector<uint64_t> hsym;  // the host paths read the symbols on the host
        if (d_sym && total) {
            hsym.resize(total);
            NMZ_HIP(hipMemcpyAsync(hsym.data(), d_sym, total * 8, hipMemcpyDeviceToHost, ctx->stream));
            NMZ_HIP(hipStreamSynchronize(ctx->stream));
            sym = hsym.data();
        }
        NMZ_CHECK(total == 0 || sym, "sym is NULL");
        std::vector<uint16_t> ids;
        std::unordered_map<uint64_t, uint32_t> dict;
        const bool fast = (want_bv || want_wide) && host_remap(sym, total, dict, ids);
        if (fast && want_bv) {
            rc = ed_plan_build_bv_host(p.get(), off, ids, dict, compact_opt);
            if (rc == 1) p.reset(new nmz_ed_plan(blank));
        }
        if (fast && want_wide) rc = ed_plan_build_wide_host(p.get(), off, ids, dict);
        if (rc == 1 && fast && tile_band && maxlen + band < MAX_FAST_LEN)
            rc = ed_plan_build_tile(p.get(), off, ids, dict);
        if (rc == 1) rc = ed_plan_build_generic(p.get(), off, sym);
    }
    NMZ_TRY(rc);
    *out = p.release();
    return NMZ_OK;
}

}  // namespace nmz
