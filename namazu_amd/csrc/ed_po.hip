// K10 -- edit scripts per entity: the partial-order (PO) view of a diff
// (historystorage/historystorage.go:50-51 is the search interface this extends, naive/naive.go:235-257 the
// reference's equality search, cli/tools/visualize.go:62-136 createTracesPerEntity / tracesEqualInPO: an empty PO
// script <=> tracesEqualInPO).
//
// The semantics are DESIGN.md section 2, "Edit scripts per entity": every trace is projected onto its entities
// (ids global to the store, < n_entities <= NMZ_PO_MAX_ENTITIES, NMZ_NONE skipped), each entity's pair of projections
// is aligned by K8 / K8w (ed_align.hip, ed_align_wide.hip) as it is, and the per-entity scripts are concatenated in
// ascending entity order with their positions lifted back to the whole traces: dist = min(sum_g Lev(a|g, b|g), w + 1).
//
// k_po_project<COUNT>: the stable partition of every trace by entity. One wave per
// trace, four traces per workgroup, grid-striding; the wave keeps cnt[n_entities] in LDS and walks its trace 64
// elements at a time. Per chunk a match-any loop -- the id of the first unserved lane, one ballot of the lanes that
// hold it -- gives every lane the mask of its group: rank = cnt[id] + popcount(mask below the lane), and the
// group's last lane adds popcount(mask) to the counter. The count pass writes cnt[t][g] (as uint64, into poff), one
// hipcub exclusive sum over the n_traces * n_entities + 1 words turns them into poff, and the scatter pass -- its
// counters started at the trace's offsets -- writes psym[q] and psrc[q] at q = poff[t G + g] + rank. Elements whose
// id is NMZ_NONE or >= n_entities are dropped and never index anything.
// k_po_subpairs (K10c): sub-pair q = p G + g is the pair of projected traces (ia G + g, ib G + g).
// k_po_gather (K10d): one workgroup per pair. The G sub-distances are summed and scanned (four per thread, a wave
// scan, the waves' sums through LDS); slot s of the pair finds its entity by binary search in the scanned starts and
// copies that sub-script's op with both positions lifted through psrc / poff and the original offsets. Sentinels
// behind the ops, and in every slot when a sub-pair is NMZ_NONE or the sum is beyond the band. Plain vector stores.
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <new>
#include <string>
#include <vector>

#include "ed_plan.h"
#include "nmz_common.h"
#include "nmz_internal.h"

namespace nmz {

constexpr uint32_t PO_WAVES = 4, PO_THREADS = 64 * PO_WAVES;
constexpr uint32_t PO_C = NMZ_PO_MAX_ENTITIES / PO_THREADS;  // entities per thread of k_po_gather
constexpr size_t PO_SUB_BUDGET = (size_t)256 << 20;          // the sub-pair ops of one launch
constexpr uint32_t PO_BLOCKS_PER_CU = 8;       // k_po_subpairs, k_po_gather
constexpr uint32_t PO_PROJECT_BLOCKS_PER_CU = 2;  // k_po_project: 8 traces in flight per CU, two chunks each
static_assert(NMZ_PO_MAX_ENTITIES == 1024 && PO_C * PO_THREADS == NMZ_PO_MAX_ENTITIES,
              "k_po_gather scans four entities per thread; 4 waves x 1,024 counters are 16 KiB of LDS");

struct PoProjArgs {
    const uint64_t *off, *sym;
    const uint32_t *ent;
    uint32_t n_traces, G;
    uint64_t *poff;  // [n_traces * G + 1]: the count pass writes the counts, the scatter pass reads the offsets
    uint64_t *psym;
    uint32_t *psrc;
};

template <bool COUNT>
__global__ __launch_bounds__(PO_THREADS) void k_po_project(const PoProjArgs g) {
    extern __shared__ uint32_t po_lds[];
    const uint32_t wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    // the wave's own counters (LDS ops of one wave execute in order; compiler barriers keep the order in the code)
    uint32_t *cnt = po_lds + (size_t)wv * g.G;
    const uint64_t below = (1ull << lane) - 1;
    for (uint64_t t = (uint64_t)blockIdx.x * PO_WAVES + wv; t < g.n_traces; t += (uint64_t)gridDim.x * PO_WAVES) {
        uint64_t *row = g.poff + t * g.G;
        const uint64_t row0 = COUNT ? 0 : row[0];
        for (uint32_t i = lane; i < g.G; i += 64) cnt[i] = COUNT ? 0u : (uint32_t)(row[i] - row0);
        __asm__ volatile("" ::: "memory");
        const uint64_t lo = g.off[t], hi = g.off[t + 1];
        const uint64_t n = hi > lo ? hi - lo : 0;
        // the next chunk's loads are issued before this chunk's ranks: their latency overlaps the match-any loop
        uint32_t e_next = lane < n ? g.ent[lo + lane] : NMZ_NONE;
        uint64_t s_next = 0;
        if (!COUNT) s_next = lane < n ? g.sym[lo + lane] : 0;
        for (uint64_t c = 0; c < n; c += 64) {
            const uint64_t i = c + lane;
            const uint32_t e0 = e_next;  // NMZ_NONE past the trace's end
            const uint64_t s = s_next;
            const uint64_t in = i + 64;
            e_next = in < n ? g.ent[lo + in] : NMZ_NONE;
            if (!COUNT) s_next = in < n ? g.sym[lo + in] : 0;
            const bool take = e0 < g.G;  // NMZ_NONE and ids past the bound are dropped
            const uint32_t e = take ? e0 : 0u;
            // match-any: the lanes that hold this lane's id
            uint64_t todo = __builtin_amdgcn_ballot_w64(take), same = 0;
            while (todo) {  // wave-uniform
                const int first = __builtin_amdgcn_readfirstlane(__ffsll((unsigned long long)todo) - 1);
                const uint32_t cur = (uint32_t)__builtin_amdgcn_readlane((int)e, first);
                const bool mine = take && e == cur;
                const uint64_t m = __builtin_amdgcn_ballot_w64(mine);
                same = mine ? m : same;
                todo &= ~m;
            }
            if (take) {
                const uint32_t before = cnt[e];
                if (!COUNT) {
                    const uint64_t q = row0 + before + (uint32_t)__popcll(same & below);
                    g.psym[q] = s;
                    g.psrc[q] = (uint32_t)i;
                }
                // every lane of the wave has read (one LDS instruction) before the group's last lane stores
                __asm__ volatile("" ::: "memory");
                if ((same >> lane) == 1ull) cnt[e] = before + (uint32_t)__popcll(same);
            }
            __asm__ volatile("" ::: "memory");
        }
        if (COUNT) {
            __asm__ volatile("" ::: "memory");
            for (uint32_t i = lane; i < g.G; i += 64) row[i] = cnt[i];
        }
        __asm__ volatile("" ::: "memory");  // the next trace's clear follows this trace's reads
    }
}

__global__ __launch_bounds__(256) void k_po_subpairs(const uint32_t *__restrict__ pairs, uint64_t n_pairs, uint32_t G,
                                                     uint32_t *__restrict__ sub) {
    const uint64_t total = n_pairs * G;
    for (uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; q < total; q += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t p = q / G;
        const uint32_t e = (uint32_t)(q - p * G);
        sub[2 * q] = pairs[2 * p] * G + e;
        sub[2 * q + 1] = pairs[2 * p + 1] * G + e;
    }
}

struct PoGatherArgs {
    const uint64_t *off, *poff;
    const uint32_t *psrc, *pairs;
    uint64_t n_pairs;
    uint32_t G, band;
    const uint32_t *sub_dist;    // [n_pairs * G]
    const nmz_edit_op *sub_ops;  // [n_pairs * G][band]
    uint32_t *dist;
    nmz_edit_op *ops;
};

__global__ __launch_bounds__(PO_THREADS) void k_po_gather(const PoGatherArgs g) {
    __shared__ uint32_t s_start[NMZ_PO_MAX_ENTITIES + 1];  // the exclusive scan of the sub-distances; [>= G]: the sum
    __shared__ uint32_t s_wsum[PO_WAVES];
    const uint32_t tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const uint32_t band = g.band, G = g.G;
    for (uint64_t p = blockIdx.x; p < g.n_pairs; p += gridDim.x) {
        uint32_t d[PO_C], loc = 0;
        bool none = false;
#pragma unroll
        for (uint32_t c = 0; c < PO_C; ++c) {
            const uint32_t e = tid * PO_C + c;
            const uint32_t v = e < G ? g.sub_dist[p * G + e] : 0u;
            none = none || v == NMZ_NONE;
            d[c] = min(v, band + 1);  // the sum stays below 2^21
            loc += d[c];
        }
        uint32_t inc = loc;
#pragma unroll
        for (uint32_t o = 1; o < 64; o <<= 1) {
            const uint32_t u = __shfl_up(inc, o, 64);
            inc += lane >= o ? u : 0u;
        }
        if (lane == 63) s_wsum[wv] = inc;
        const int any_none = __syncthreads_or(none ? 1 : 0);  // the waves' sums are in LDS behind this barrier
        uint32_t wbase = 0, total = 0;
#pragma unroll
        for (uint32_t v = 0; v < PO_WAVES; ++v) {
            wbase += v < wv ? s_wsum[v] : 0u;
            total += s_wsum[v];
        }
        uint32_t excl = wbase + inc - loc;
#pragma unroll
        for (uint32_t c = 0; c < PO_C; ++c) {
            s_start[tid * PO_C + c] = excl;
            excl += d[c];
        }
        if (tid == PO_THREADS - 1) s_start[NMZ_PO_MAX_ENTITIES] = excl;
        __syncthreads();
        const bool live = !any_none && total <= band;
        if (tid == 0) g.dist[p] = any_none ? NMZ_NONE : (total > band ? band + 1 : total);
        const uint32_t ia = g.pairs[2 * p], ib = g.pairs[2 * p + 1];
        const uint64_t alo = g.off[ia], ahi = g.off[ia + 1], blo = g.off[ib], bhi = g.off[ib + 1];
        const uint32_t n = (uint32_t)(ahi > alo ? ahi - alo : 0), m = (uint32_t)(bhi > blo ? bhi - blo : 0);
        for (uint32_t s = tid; s < band; s += PO_THREADS) {
            nmz_edit_op o{NMZ_NONE, NMZ_NONE, NMZ_NONE};
            if (live && s < total) {
                // the entity of slot s: the last e with start[e] <= s (its sub-script is not empty)
                uint32_t lo = 0, len = G;
                while (len > 0) {
                    const uint32_t h = len >> 1;
                    if (s_start[lo + h] <= s) {
                        lo += h + 1;
                        len -= h + 1;
                    } else {
                        len = h;
                    }
                }
                const uint32_t e = lo - 1;  // start[0] = 0 <= s
                const nmz_edit_op src = g.sub_ops[(p * G + e) * band + (s - s_start[e])];
                const uint64_t qa = (uint64_t)ia * G + e, qb = (uint64_t)ib * G + e;
                const uint64_t a0 = g.poff[qa], a1 = g.poff[qa + 1], b0 = g.poff[qb], b1 = g.poff[qb + 1];
                o.a_pos = src.a_pos < a1 - a0 ? g.psrc[a0 + src.a_pos] : n;
                o.b_pos = src.b_pos < b1 - b0 ? g.psrc[b0 + src.b_pos] : m;
                o.kind = src.kind;
            }
            g.ops[p * band + s] = o;
        }
        __syncthreads();  // the next pair's scan writes s_start and s_wsum
    }
}

// ---- the limits, no device ----
static int po_n_entities(uint32_t G) {
    NMZ_CHECK(G >= 1 && G <= NMZ_PO_MAX_ENTITIES,
              "n_entities " + std::to_string(G) + " must be 1 .. NMZ_PO_MAX_ENTITIES (1024)");
    return NMZ_OK;
}

static int po_ids(const uint32_t *ent, uint64_t n, uint32_t G, const std::string &what) {
    for (uint64_t i = 0; i < n; ++i)
        NMZ_CHECK(ent[i] < G || ent[i] == NMZ_NONE,
                  what + " " + std::to_string(i) + " has entity id " + std::to_string(ent[i]) +
                      ": ids are < n_entities (" + std::to_string(G) + ") or NMZ_NONE");
    return NMZ_OK;
}

// the projected CSR's trace ids (t * G + g) are pair indexes of the aligners and items of one hipcub scan
static int po_store(uint32_t n_traces, uint32_t G) {
    NMZ_CHECK((uint64_t)n_traces * G < (1ull << 31) - 1,
              "n_traces * n_entities = " + std::to_string(n_traces) + " * " + std::to_string(G) +
                  " must stay below 2^31 - 1: the projected traces are indexed with 32 bits");
    return NMZ_OK;
}

// entity, n_entities and the ids of a store, behind the aligner's own checks
static int po_validate(const uint64_t *off, const uint32_t *entity, uint32_t n_traces, uint32_t G) {
    const uint64_t total = off ? off[n_traces] : 0;
    NMZ_CHECK(total == 0 || entity, "entity is NULL");
    NMZ_TRY(po_n_entities(G));
    if (total) NMZ_TRY(po_ids(entity, total, G, "element"));
    return po_store(n_traces, G);
}

// the longest projection of the traces that the pairs name
static uint64_t po_max_len(const uint64_t *off, const uint32_t *entity, uint32_t n_traces, uint32_t G,
                           const uint32_t *pairs, uint64_t n_pairs) {
    std::vector<uint8_t> used(n_traces, 0);
    for (uint64_t t = 0; t < 2 * n_pairs; ++t) used[pairs[t]] = 1;
    std::vector<uint64_t> cnt(G);
    uint64_t longest = 0;
    for (uint32_t t = 0; t < n_traces; ++t) {
        if (!used[t]) continue;
        std::fill(cnt.begin(), cnt.end(), 0);
        for (uint64_t i = off[t]; i < off[t + 1]; ++i)
            if (entity[i] != NMZ_NONE) longest = std::max(longest, ++cnt[entity[i]]);
    }
    return longest;
}

// K10a, the scan and K10b on `st`; the scan's temporary is the context's SLOT_PO_SCAN. The caller holds ctx.
// (Also ed_po_knn.hip's projection of its store and of its queries: declared in ed_plan.h.)
int po_project_enqueue(nmz_ctx *ctx, hipStream_t st, const uint64_t *d_off, const uint64_t *d_sym,
                       const uint32_t *d_ent, uint32_t n_traces, uint32_t G, uint64_t *d_poff, uint64_t *d_psym,
                       uint32_t *d_psrc) {
    NMZ_TRY(po_n_entities(G));
    NMZ_TRY(po_store(n_traces, G));
    NMZ_CHECK(d_poff != nullptr, "d_poff is NULL");
    const uint64_t items = (uint64_t)n_traces * G + 1;
    if (n_traces == 0) {
        NMZ_HIP(hipMemsetAsync(d_poff, 0, sizeof(uint64_t), st));
        return NMZ_OK;
    }
    NMZ_CHECK(d_off && d_sym && d_ent && d_psym && d_psrc, "d_off, d_sym, d_entity, d_psym or d_psrc is NULL");
    size_t scan_bytes = 0;
    NMZ_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, scan_bytes, (uint64_t *)nullptr, (uint64_t *)nullptr, (int)items,
                                             st));
    char *tmp;
    ScratchLayout lay;
    lay.add(&tmp, scan_bytes + 1);
    NMZ_TRY(lay.bind(ctx->buf[SLOT_PO_SCAN]));
    const PoProjArgs a{d_off, d_sym, d_ent, n_traces, G, d_poff, d_psym, d_psrc};
    const unsigned blocks = (unsigned)std::min<uint64_t>(((uint64_t)n_traces + PO_WAVES - 1) / PO_WAVES,
                                                         (uint64_t)std::max(ctx->n_cu, 1) * PO_PROJECT_BLOCKS_PER_CU);
    const size_t lds = (size_t)PO_WAVES * G * sizeof(uint32_t);
    {
        KernelTimer kt(ctx, st, "po_count");
        hipLaunchKernelGGL(k_po_project<true>, dim3(blocks), dim3(PO_THREADS), lds, st, a);
        if (hipGetLastError() != hipSuccess) return fail(NMZ_EHIP, "k_po_project (count) launch failed");
    }
    NMZ_HIP(hipMemsetAsync(d_poff + (items - 1), 0, sizeof(uint64_t), st));
    {
        KernelTimer kt(ctx, st, "po_scan");
        NMZ_HIP(hipcub::DeviceScan::ExclusiveSum(tmp, scan_bytes, d_poff, d_poff, (int)items, st));
    }
    {
        KernelTimer kt(ctx, st, "po_scatter");
        hipLaunchKernelGGL(k_po_project<false>, dim3(blocks), dim3(PO_THREADS), lds, st, a);
        if (hipGetLastError() != hipSuccess) return fail(NMZ_EHIP, "k_po_project (scatter) launch failed");
    }
    return NMZ_OK;
}

}  // namespace nmz

struct nmz_ed_align_po_plan {
    nmz_ctx *ctx = nullptr;
    uint32_t band = 0, G = 0;
    uint64_t max_pairs = 0;
    nmz_ed_align_wide_plan *inner = nullptr;  // aligns the sub-pairs
    nmz::DevBuf sub;                          // sub_pairs, sub_dist, sub_ops for max_pairs pairs
    uint32_t *sub_pairs = nullptr, *sub_dist = nullptr;
    nmz_edit_op *sub_ops = nullptr;
    size_t sub_bytes = 0;
    nmz::PlanFence fence;  // the sub-pair scratch serves one stream at a time
};

namespace nmz {

static void po_plan_destroy_locked(nmz_ed_align_po_plan *p) {
    p->fence.destroy();
    if (p->inner) aw_plan_destroy_locked(p->inner);
    p->sub.release();
    delete p;
}

// the plan's limits, no device: *slot_words = the inner plan's shape
static int po_plan_shape(uint32_t band, uint32_t G, uint64_t max_len, uint64_t max_pairs, uint64_t *slot_words) {
    NMZ_TRY(aw_band(band));
    NMZ_TRY(po_n_entities(G));
    NMZ_CHECK(max_pairs >= 1, "max_pairs is 0");
    NMZ_CHECK(max_pairs <= (SIZE_MAX / sizeof(nmz_edit_op)) / NMZ_ALIGN_WIDE_MAX_BAND / NMZ_PO_MAX_ENTITIES,
              "max_pairs * n_entities * band does not fit the sub-pair scratch");
    return aw_shape(band, max_len, slot_words);
}

static int po_plan_create_locked(nmz_ctx *ctx, uint32_t band, uint32_t G, uint64_t max_len, uint64_t max_pairs,
                                 uint64_t slot_words, nmz_ed_align_po_plan **out) {
    auto *p = new nmz_ed_align_po_plan();
    p->ctx = ctx;
    p->band = band;
    p->G = G;
    p->max_pairs = max_pairs;
    int rc = aw_plan_create_locked(ctx, band, max_len, slot_words, &p->inner);
    if (rc == NMZ_OK) {
        const size_t subs = (size_t)max_pairs * G;
        ScratchLayout lay;
        lay.add(&p->sub_pairs, 2 * subs).add(&p->sub_dist, subs).add(&p->sub_ops, subs * band + 1);
        p->sub.pool = &ctx->pool;
        rc = lay.bind(p->sub);
        p->sub_bytes = lay.bytes();
    }
    if (rc == NMZ_OK) rc = p->fence.create("align po plan");
    if (rc != NMZ_OK) {
        po_plan_destroy_locked(p);
        return rc;
    }
    *out = p;
    return NMZ_OK;
}

// K10c, the aligner and K10d on `st`, nothing else. The caller holds the context.
static int po_enqueue(nmz_ed_align_po_plan *p, hipStream_t st, const uint64_t *d_off, const uint64_t *d_poff,
                      const uint64_t *d_psym, const uint32_t *d_psrc, const uint32_t *d_pairs, uint64_t n_pairs,
                      uint32_t *d_dist, nmz_edit_op *d_ops) {
    NMZ_CHECK(n_pairs <= p->max_pairs, "n_pairs " + std::to_string(n_pairs) + " exceeds the plan's max_pairs (" +
                                           std::to_string(p->max_pairs) + ")");
    if (n_pairs == 0) return NMZ_OK;
    NMZ_CHECK(d_off && d_poff && d_psym && d_psrc && d_pairs && d_dist,
              "d_off, d_poff, d_psym, d_psrc, d_pairs or d_dist is NULL");
    NMZ_CHECK(p->band == 0 || d_ops, "d_ops is NULL");
    NMZ_TRY(p->fence.enter(st));
    const uint64_t subs = n_pairs * p->G;
    const unsigned cap = (unsigned)std::max(p->ctx->n_cu, 1) * PO_BLOCKS_PER_CU;
    hipLaunchKernelGGL(k_po_subpairs, dim3((unsigned)std::min<uint64_t>((subs + 255) / 256, cap)), dim3(256), 0, st,
                       d_pairs, n_pairs, p->G, p->sub_pairs);
    if (hipGetLastError() != hipSuccess) return fail(NMZ_EHIP, "k_po_subpairs launch failed");
    NMZ_TRY(aw_enqueue(p->inner, st, d_poff, d_psym, p->sub_pairs, subs, p->sub_dist, p->sub_ops));
    int rc = NMZ_OK;
    {
        const PoGatherArgs a{d_off, d_poff, d_psrc, d_pairs, n_pairs, p->G, p->band, p->sub_dist, p->sub_ops, d_dist, d_ops};
        KernelTimer kt(p->ctx, st, "po_gather");
        hipLaunchKernelGGL(k_po_gather, dim3((unsigned)std::min<uint64_t>(n_pairs, cap)), dim3(PO_THREADS), 0, st, a);
        if (hipGetLastError() != hipSuccess) rc = fail(NMZ_EHIP, "k_po_gather launch failed");
    }
    NMZ_TRY(p->fence.leave(st));
    return rc;
}

// pairs per launch of the host forms: the sub-pair ops stay within PO_SUB_BUDGET
static uint64_t po_batch(uint64_t n_pairs, uint32_t G, uint32_t band) {
    const uint64_t per_pair = (uint64_t)G * std::max(band, 1u) * sizeof(nmz_edit_op);
    return std::min<uint64_t>(n_pairs, std::max<uint64_t>(1, PO_SUB_BUDGET / per_pair));
}

}  // namespace nmz

using namespace nmz;

extern "C" {

// One pair on the calling thread (historystorage.go:50-51, naive.go:235-257, visualize.go:62-136): plain vectors per
// entity, nmz_ed_align_wide_host per entity, lift, concatenate. Nothing shared with K10.
int nmz_ed_align_po_host(const uint64_t *a, const uint32_t *ea, uint64_t n, const uint64_t *b, const uint32_t *eb,
                         uint64_t m, uint32_t n_entities, uint32_t band, uint32_t *dist, nmz_edit_op *ops) {
    NMZ_TRY(aw_band(band));
    NMZ_CHECK(n < 0xFFFFFFFFull, "a has " + std::to_string(n) + " elements: at most 2^32 - 2");
    NMZ_CHECK(m < 0xFFFFFFFFull, "b has " + std::to_string(m) + " elements: at most 2^32 - 2");
    NMZ_CHECK((n == 0 || a) && (m == 0 || b), "a or b is NULL");
    NMZ_CHECK(dist != nullptr, "dist is NULL");
    NMZ_CHECK(band == 0 || ops, "ops is NULL");
    NMZ_CHECK((n == 0 || ea) && (m == 0 || eb), "entity is NULL");
    NMZ_TRY(po_n_entities(n_entities));
    NMZ_TRY(po_ids(ea, n, n_entities, "a's element"));
    NMZ_TRY(po_ids(eb, m, n_entities, "b's element"));
    for (uint32_t s = 0; s < band; ++s) ops[s] = nmz_edit_op{NMZ_NONE, NMZ_NONE, NMZ_NONE};
    std::vector<std::vector<uint64_t>> pa(n_entities), pb(n_entities);
    std::vector<std::vector<uint32_t>> sa(n_entities), sb(n_entities);
    for (uint64_t i = 0; i < n; ++i)
        if (ea[i] != NMZ_NONE) pa[ea[i]].push_back(a[i]), sa[ea[i]].push_back((uint32_t)i);
    for (uint64_t j = 0; j < m; ++j)
        if (eb[j] != NMZ_NONE) pb[eb[j]].push_back(b[j]), sb[eb[j]].push_back((uint32_t)j);
    std::vector<nmz_edit_op> part(band), all;
    uint64_t sum = 0;
    for (uint32_t g = 0; g < n_entities; ++g) {
        if (pa[g].empty() && pb[g].empty()) continue;
        uint32_t d = 0;
        NMZ_TRY(nmz_ed_align_wide_host(pa[g].data(), pa[g].size(), pb[g].data(), pb[g].size(), band, &d, part.data()));
        sum += d;
        if (sum > band) {  // one Lev_g > band, or the sum: beyond
            *dist = band + 1;
            return NMZ_OK;
        }
        for (uint32_t s = 0; s < d; ++s) {
            const nmz_edit_op &o = part[s];
            all.push_back(nmz_edit_op{o.a_pos < sa[g].size() ? sa[g][o.a_pos] : (uint32_t)n,
                                      o.b_pos < sb[g].size() ? sb[g][o.b_pos] : (uint32_t)m, o.kind});
        }
    }
    *dist = (uint32_t)sum;
    for (size_t s = 0; s < all.size(); ++s) ops[s] = all[s];
    return NMZ_OK;
}

int nmz_po_project_dev(nmz_ctx *ctx, const uint64_t *d_off, const uint64_t *d_sym, const uint32_t *d_entity,
                       uint32_t n_traces, uint32_t n_entities, uint64_t *d_poff, uint64_t *d_psym, uint32_t *d_psrc,
                       void *stream) {
    NMZ_CHECK(ctx != nullptr, "ctx is NULL");
    CtxGuard g(ctx);
    NMZ_TRY(g.rc);
    return po_project_enqueue(ctx, stream ? (hipStream_t)stream : ctx->stream, d_off, d_sym, d_entity, n_traces,
                              n_entities, d_poff, d_psym, d_psrc);
}

int nmz_po_project(nmz_ctx *ctx, const uint64_t *off, const uint64_t *sym, const uint32_t *entity, uint32_t n_traces,
                   uint32_t n_entities, uint64_t *poff, uint64_t *psym, uint32_t *psrc) {
    // the arguments first: they are checked without a device
    NMZ_CHECK(off && poff, "off or poff is NULL");
    for (uint32_t t = 0; t < n_traces; ++t)
        NMZ_CHECK(off[t] <= off[t + 1], "offsets must be non-decreasing (trace " + std::to_string(t) + ")");
    const uint64_t total = off[n_traces];
    NMZ_CHECK(total == 0 || sym, "sym is NULL");
    NMZ_TRY(po_validate(off, entity, n_traces, n_entities));
    uint64_t kept = 0;
    for (uint64_t i = 0; i < total; ++i) kept += entity[i] != NMZ_NONE;
    NMZ_CHECK(kept == 0 || (psym && psrc), "psym or psrc is NULL");
    if (n_traces == 0) {  // no device
        poff[0] = 0;
        return NMZ_OK;
    }
    NMZ_CHECK(ctx != nullptr, "ctx is NULL");
    CtxGuard g(ctx);
    NMZ_TRY(g.rc);
    HostCall call(ctx);
    hipStream_t st = ctx->stream;
    const size_t items = (size_t)n_traces * n_entities + 1;
    uint64_t *d_off, *d_sym, *d_poff, *d_psym;
    uint32_t *d_ent, *d_psrc;
    ScratchLayout lay;
    lay.add(&d_off, n_traces + 1).add(&d_sym, total + 1).add(&d_ent, total + 1).add(&d_poff, items);
    lay.add(&d_psym, total + 1).add(&d_psrc, total + 1);
    NMZ_TRY(lay.bind(call.work));
    NMZ_TRY(upload_csr(d_off, d_sym, off, sym, n_traces, st));
    NMZ_TRY(copy_h2d(d_ent, entity, total, st));
    NMZ_TRY(po_project_enqueue(ctx, st, d_off, d_sym, d_ent, n_traces, n_entities, d_poff, d_psym, d_psrc));
    NMZ_TRY(copy_d2h(poff, d_poff, items, st));
    NMZ_TRY(copy_d2h(psym, d_psym, kept, st));
    NMZ_TRY(copy_d2h(psrc, d_psrc, kept, st));
    return call.done();
}

int nmz_ed_align_po_plan_create(nmz_ctx *ctx, uint32_t band, uint32_t n_entities, uint64_t max_len, uint64_t max_pairs,
                                nmz_ed_align_po_plan **out) {
    NMZ_CHECK(out != nullptr, "out is NULL");
    *out = nullptr;
    uint64_t slot_words = 0;
    NMZ_TRY(po_plan_shape(band, n_entities, max_len, max_pairs, &slot_words));
    NMZ_CHECK(ctx != nullptr, "ctx is NULL");
    CtxGuard g(ctx);
    NMZ_TRY(g.rc);
    return po_plan_create_locked(ctx, band, n_entities, max_len, max_pairs, slot_words, out);
}

int nmz_ed_align_po_plan_destroy(nmz_ed_align_po_plan *plan) {
    if (!plan) return NMZ_OK;
    CtxGuard g(plan->ctx);
    NMZ_TRY(g.rc);
    po_plan_destroy_locked(plan);
    return NMZ_OK;
}

int nmz_ed_align_po_plan_info(const nmz_ed_align_po_plan *plan, uint32_t *slots, uint64_t *history_bytes,
                              uint64_t *sub_pair_bytes) {
    NMZ_CHECK(plan != nullptr, "plan is NULL");
    if (sub_pair_bytes) *sub_pair_bytes = plan->sub_bytes;
    return nmz_ed_align_wide_plan_info(plan->inner, slots, history_bytes);
}

int nmz_ed_align_po_pairs_dev(nmz_ed_align_po_plan *plan, const uint64_t *d_off, const uint64_t *d_poff,
                              const uint64_t *d_psym, const uint32_t *d_psrc, const uint32_t *d_pairs, uint64_t n_pairs,
                              uint32_t *d_dist, nmz_edit_op *d_ops, void *stream) {
    NMZ_CHECK(plan != nullptr, "plan is NULL");
    CtxGuard g(plan->ctx);
    NMZ_TRY(g.rc);
    return po_enqueue(plan, stream ? (hipStream_t)stream : plan->ctx->stream, d_off, d_poff, d_psym, d_psrc, d_pairs,
                      n_pairs, d_dist, d_ops);
}

int nmz_ed_align_po_pairs(nmz_ctx *ctx, const uint64_t *off, const uint64_t *sym, const uint32_t *entity,
                          uint32_t n_traces, uint32_t n_entities, const uint32_t *pairs, uint64_t n_pairs,
                          uint32_t band, uint32_t *dist, nmz_edit_op *ops) {
    // the arguments first: they are checked without a device
    uint64_t max_len = 0, slot_words = 0;
    NMZ_TRY(aw_validate(off, sym, n_traces, pairs, n_pairs, band, dist, ops, &max_len));
    NMZ_TRY(po_n_entities(n_entities));
    if (n_pairs == 0) return NMZ_OK;  // nothing to write: no device either
    NMZ_TRY(po_validate(off, entity, n_traces, n_entities));
    const uint64_t total = off[n_traces];
    max_len = total ? po_max_len(off, entity, n_traces, n_entities, pairs, n_pairs) : 0;
    const uint64_t batch = po_batch(n_pairs, n_entities, band);
    NMZ_TRY(po_plan_shape(band, n_entities, max_len, batch, &slot_words));
    NMZ_CHECK(ctx != nullptr, "ctx is NULL");
    CtxGuard g(ctx);
    NMZ_TRY(g.rc);
    HostCall call(ctx);
    nmz_ed_align_po_plan *plan = nullptr;
    NMZ_TRY(po_plan_create_locked(ctx, band, n_entities, max_len, batch, slot_words, &plan));
    call.own_plan<po_plan_destroy_locked>(plan);
    hipStream_t st = ctx->stream;
    const size_t n_ops = (size_t)n_pairs * band;
    uint64_t *d_off, *d_sym, *d_poff, *d_psym;
    uint32_t *d_ent, *d_psrc, *d_pairs, *d_dist;
    nmz_edit_op *d_ops;
    ScratchLayout lay;
    lay.add(&d_off, n_traces + 1).add(&d_sym, total + 1).add(&d_ent, total + 1);
    lay.add(&d_poff, (size_t)n_traces * n_entities + 1).add(&d_psym, total + 1).add(&d_psrc, total + 1);
    lay.add(&d_pairs, 2 * n_pairs).add(&d_dist, n_pairs).add(&d_ops, n_ops + 1);
    NMZ_TRY(lay.bind(call.work));
    NMZ_TRY(upload_csr(d_off, d_sym, off, sym, n_traces, st));
    NMZ_TRY(copy_h2d(d_ent, entity, total, st));
    NMZ_TRY(copy_h2d(d_pairs, pairs, 2 * n_pairs, st));
    NMZ_TRY(po_project_enqueue(ctx, st, d_off, d_sym, d_ent, n_traces, n_entities, d_poff, d_psym, d_psrc));
    for (uint64_t p0 = 0; p0 < n_pairs; p0 += batch)
        NMZ_TRY(po_enqueue(plan, st, d_off, d_poff, d_psym, d_psrc, d_pairs + 2 * p0, std::min(batch, n_pairs - p0),
                           d_dist + p0, d_ops + p0 * band));
    NMZ_TRY(copy_d2h(dist, d_dist, n_pairs, st));
    NMZ_TRY(copy_d2h(ops, d_ops, n_ops, st));
    return call.done();
}

int nmz_ed_diff_profile_po(nmz_ctx *ctx, const uint64_t *off, const uint64_t *sym, const uint32_t *entity,
                           uint32_t n_traces, uint32_t n_entities, const uint32_t *pairs, uint64_t n_pairs,
                           uint32_t band, const uint64_t *usym, uint64_t n_usym, uint32_t *dist,
                           nmz_move_counts *counts, nmz_move_info *info) {
    // the arguments first: they are checked without a device
    uint64_t max_len = 0, slot_words = 0;
    NMZ_TRY(moves_validate(aw_band, aw_validate, off, sym, n_traces, pairs, n_pairs, band, dist, nullptr, false, usym,
                           n_usym, counts, info, &max_len));
    NMZ_TRY(po_n_entities(n_entities));
    if (n_pairs == 0) {  // all zero: no device either
        moves_zero(counts, n_usym, info);
        return NMZ_OK;
    }
    NMZ_TRY(po_validate(off, entity, n_traces, n_entities));
    const uint64_t total = off[n_traces];
    max_len = total ? po_max_len(off, entity, n_traces, n_entities, pairs, n_pairs) : 0;
    const uint64_t batch = po_batch(n_pairs, n_entities, band);
    NMZ_TRY(po_plan_shape(band, n_entities, max_len, batch, &slot_words));
    NMZ_CHECK(ctx != nullptr, "ctx is NULL");
    CtxGuard g(ctx);
    NMZ_TRY(g.rc);
    HostCall call(ctx);
    nmz_ed_align_po_plan *plan = nullptr;
    NMZ_TRY(po_plan_create_locked(ctx, band, n_entities, max_len, batch, slot_words, &plan));
    call.own_plan<po_plan_destroy_locked>(plan);
    hipStream_t st = ctx->stream;
    uint64_t *d_off, *d_sym, *d_poff, *d_psym, *d_usym;
    uint32_t *d_ent, *d_psrc, *d_pairs, *d_dist;
    nmz_edit_op *d_ops;  // one batch's scripts: they never leave the device
    nmz_move_counts *d_counts;
    nmz_move_info *d_info;
    ScratchLayout lay;
    lay.add(&d_off, n_traces + 1).add(&d_sym, total + 1).add(&d_ent, total + 1);
    lay.add(&d_poff, (size_t)n_traces * n_entities + 1).add(&d_psym, total + 1).add(&d_psrc, total + 1);
    lay.add(&d_pairs, 2 * n_pairs).add(&d_dist, n_pairs).add(&d_ops, (size_t)batch * band + 1);
    lay.add(&d_usym, n_usym + 1).add(&d_counts, n_usym + 1).add(&d_info, 1);
    NMZ_TRY(lay.bind(call.work));
    NMZ_TRY(upload_csr(d_off, d_sym, off, sym, n_traces, st));
    NMZ_TRY(copy_h2d(d_ent, entity, total, st));
    NMZ_TRY(copy_h2d(d_pairs, pairs, 2 * n_pairs, st));
    NMZ_TRY(copy_h2d(d_usym, usym, n_usym, st));
    NMZ_TRY(po_project_enqueue(ctx, st, d_off, d_sym, d_ent, n_traces, n_entities, d_poff, d_psym, d_psrc));
    for (uint64_t p0 = 0; p0 < n_pairs; p0 += batch) {
        const uint64_t nb = std::min(batch, n_pairs - p0);
        NMZ_TRY(po_enqueue(plan, st, d_off, d_poff, d_psym, d_psrc, d_pairs + 2 * p0, nb, d_dist + p0, d_ops));
        const MvArgs a{d_off, d_sym, d_pairs + 2 * p0, nb, band, d_dist + p0, d_ops, d_usym, n_usym, nullptr, d_counts,
                       d_info};
        NMZ_TRY(moves_wide_enqueue(ctx, st, a, p0 > 0));
    }
    if (dist) NMZ_TRY(copy_d2h(dist, d_dist, n_pairs, st));
    NMZ_TRY(copy_d2h(counts, d_counts, n_usym, st));
    NMZ_TRY(copy_d2h(info, d_info, 1, st));
    return call.done();
}

}  // extern "C"
