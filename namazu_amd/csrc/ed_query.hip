// K3 single queries (nmz_ed_plan_query_knn) against a plan's resident store: k_ed_bv_query (ed_bv.hip) on a
// bit-parallel plan, k_ed_wide_query (ed_wide.hip) on a wide plan, the generic kernel here on the other plans and for
// the queries those two cannot take.
#include <algorithm>

#include "ed_generic_dev.h"
#include "ed_knn_dev.h"
#include "ed_plan.h"

namespace nmz {

// Single queries against a resident store without a bit-parallel query kernel (k_ed_tile's dense ids, the generic
// plan's u64 symbols, or a bit-parallel plan's encoded streams when a query pair's symbols overflow the compact
// tables): thread per (query, stored trace) pair; stored trace j at sym[soff[j]], length slen[j] (or the CSR
// difference when slen is NULL); in-band results into the query's list
__global__ __launch_bounds__(256) void k_ed_query_generic(const uint64_t *__restrict__ soff,
                                                          const uint32_t *__restrict__ slen, const void *__restrict__ sym,
                                                          bool wide_sym, const uint64_t *__restrict__ qstart,
                                                          const uint32_t *__restrict__ qlen, const void *__restrict__ qsym,
                                                          uint32_t n_q, uint32_t N, uint32_t W, uint32_t k,
                                                          uint32_t *__restrict__ scratch, uint64_t *__restrict__ knn) {
    const uint64_t nthr = (uint64_t)gridDim.x * blockDim.x;
    const uint64_t tid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (uint64_t p = tid; p < (uint64_t)n_q * N; p += nthr) {
        const uint32_t q = (uint32_t)(p / N), j = (uint32_t)(p % N);
        const int64_t n = qlen[q], m = slen ? (int64_t)slen[j] : (int64_t)(soff[j + 1] - soff[j]);
        const uint32_t r = wide_sym
            ? generic_band_dist((const uint64_t *)qsym + qstart[q], n, (const uint64_t *)sym + soff[j], m, W,
                                scratch + tid, nthr)
            : generic_band_dist((const uint16_t *)qsym + qstart[q], n, (const uint16_t *)sym + soff[j], m, W,
                                scratch + tid, nthr);
        if (r <= W) knn_insert(knn + (uint64_t)q * k, k, ((uint64_t)r << 32) | j);
    }
}

// k_ed_query_generic over the resident store (soff/slen/sym as the kernel takes them) for n_q queries whose
// symbols (already in the store's encoding) are at d_qs + qstart[q], lengths qlen[q] (host arrays)
static int ed_query_generic_launch(nmz_ed_plan *plan, const uint64_t *soff, const uint32_t *slen, const void *sym,
                                   bool wide_sym, const void *d_qs, const std::vector<uint64_t> &qstart,
                                   const std::vector<uint32_t> &qlen, uint64_t *d_knn, uint32_t k) {
    hipStream_t st = plan->ctx->stream;
    const uint32_t N = plan->n, W = plan->band, n_q = (uint32_t)qlen.size();
    const unsigned threads =
        (unsigned)std::max<uint64_t>(256, std::min<uint64_t>(256 * 1024, (1ULL << 28) / (2ULL * W + 1)) / 256 * 256);
    uint64_t *d_qstart;
    uint32_t *d_qlen, *d_row;
    ScratchLayout lay;
    lay.add(&d_qstart, n_q + 1).add(&d_qlen, n_q + 1).add(&d_row, (uint64_t)(2 * W + 1) * threads);
    NMZ_TRY(lay.bind(plan->ctx->buf[SLOT_ED_QUERY_GENERIC]));
    NMZ_TRY(copy_h2d(d_qstart, qstart.data(), n_q, st));
    NMZ_TRY(copy_h2d(d_qlen, qlen.data(), n_q, st));
    KernelTimer kt(plan->ctx, st, "ed_query_generic");
    hipLaunchKernelGGL(k_ed_query_generic, dim3(threads / 256), dim3(256), 0, st, soff, slen, sym, wide_sym, d_qstart,
                       d_qlen, d_qs, n_q, N, W, k, d_row, d_knn);
    NMZ_HIP(hipGetLastError());
    NMZ_HIP(hipStreamSynchronize(st));  // pageable sources
    return NMZ_OK;
}

// nmz_ed_plan_query_knn on a bit-parallel plan: k_ed_bv_query, two queries per launch
static int ed_query_bv(nmz_ed_plan *plan, const uint64_t *q_off, const uint64_t *q_sym, uint32_t n_queries,
                       uint32_t k, uint64_t *d_knn) {
    hipStream_t st = plan->ctx->stream;
    const uint32_t N = plan->n;
    // query streams in the plan's Peq-row offsets (unknown symbols: 0xffff), each padded by one 32-block
    std::vector<uint64_t> qoff(n_queries + 1, 0);
    for (uint32_t q = 0; q < n_queries; ++q) qoff[q + 1] = qoff[q] + (q_off[q + 1] - q_off[q] + 31) / 32 * 32 + 32;
    std::vector<uint16_t> qs(qoff[n_queries] + 1, 0xffffu);
    for (uint32_t q = 0; q < n_queries; ++q)
        for (uint64_t t = q_off[q]; t < q_off[q + 1]; ++t) {
            auto it = plan->dict.find(q_sym[t]);
            if (it != plan->dict.end())
                qs[qoff[q] + (t - q_off[q])] = (uint16_t)(plan->cmp ? it->second : it->second * plan->ndw * 8);
        }
    // compact tables: each launch's rows = the two queries' distinct known symbols
    std::vector<uint32_t> qd(n_queries, 0);
    if (plan->cmp) {
        std::vector<uint32_t> stamp(plan->n_sym + 1, UINT32_MAX);
        for (uint32_t q = 0; q < n_queries; ++q)
            for (uint64_t t = qoff[q]; t < qoff[q] + (q_off[q + 1] - q_off[q]); ++t)
                if (qs[t] != 0xffffu && stamp[qs[t]] != q) {
                    stamp[qs[t]] = q;
                    ++qd[q];
                }
    }
    uint16_t *d_qs;
    ScratchLayout lay;
    NMZ_TRY(lay.add(&d_qs, qs.size()).bind(plan->ctx->buf[SLOT_ED_QUERY_FORM]));
    NMZ_TRY(copy_h2d(d_qs, qs.data(), qs.size(), st));
    std::vector<uint32_t> spill;  // queries for the generic kernel
    // a pool of 256 stored traces per workgroup: one pass of lanes, ~N/256 workgroups
    const uint32_t pool = N >= 256u * 1024u ? 1024u : 256u;
    for (uint32_t q = 0; q < n_queries && N; q += 2) {
        const uint32_t nq2 = std::min(2u, n_queries - q);
        bool longq = false;  // a query longer than the Peq tables (the longest stored trace): generic kernel
        for (uint32_t i = 0; i < nq2; ++i) longq |= q_off[q + i + 1] - q_off[q + i] > plan->maxlen;
        if (longq) {
            for (uint32_t i = 0; i < nq2; ++i) spill.push_back(q + i);
            continue;
        }
        EdBvQueryArgs A;
        A.bsym = plan->d_bsym;
        A.soff = plan->d_soff;
        A.len = plan->d_len;
        A.qs = d_qs;
        A.n_queries = std::min(2u, n_queries - q);
        for (uint32_t i = 0; i < 2; ++i) {
            const uint32_t qq = std::min(q + i, n_queries - 1);
            A.qoff[i] = qoff[qq];
            A.nq[i] = (uint32_t)(q_off[qq + 1] - q_off[qq]);
        }
        A.knn = d_knn + (uint64_t)q * k;
        A.prof = plan->qgram ? (const uint4 *)plan->d_prof : nullptr;
        A.N = N;
        A.k = k;
        A.lds_dw = plan->lds_dw;
        A.pool = pool;
        A.w = plan->band;
        A.rmap_dw = plan->rmap_dw;
        A.claim_dw = plan->claim_dw;
        A.row_bytes = plan->row_bytes;
        if (plan->cmp) {
            const uint32_t R = qd[q] + (A.n_queries > 1 ? qd[q + 1] : 0);
            if (!bv_compact_layout(plan->n_sym, R, plan->ndw, 16 + (2 * ED_QG_DW + 2 * ED_QG_BUCKETS) * 4,
                                   ED_BV_LDS_MAX, A.lds_dw, A.rmap_dw, A.claim_dw)) {
                // the pair's symbols overflow the compact tables: these queries take the generic kernel over the
                // same encoded streams (below)
                for (uint32_t i = 0; i < A.n_queries; ++i) spill.push_back(q + i);
                continue;
            }
        }
        KernelTimer kt(plan->ctx, st, "ed_bv_query");
        NMZ_TRY(ed_bv_query_launch(A, plan->bw, plan->cmp, ceil_div(N, pool), st));
    }
    // stored trace j: stream at d_bsym + soff[j], d_len[j] symbols, in the same encoding as qs (an unseen query
    // symbol, 0xffff, equals no stored entry: row byte offsets are even, compact ids < 0xfffe)
    for (const uint32_t q : spill) {
        std::vector<uint64_t> qstart{qoff[q]};
        std::vector<uint32_t> qlen{(uint32_t)(q_off[q + 1] - q_off[q])};
        NMZ_TRY(ed_query_generic_launch(plan, plan->d_soff, plan->d_len, plan->d_bsym, false, d_qs, qstart, qlen,
                                        d_knn + (uint64_t)q * k, k));
    }
    NMZ_HIP(hipStreamSynchronize(st));  // the host vectors are pageable
    return NMZ_OK;
}

// the plan's dense ids of n query symbols (`unseen` for a symbol the store has never seen)
static void query_ids(const nmz_ed_plan *plan, const uint64_t *q_sym, uint64_t n, std::vector<uint16_t> &ids,
                      uint16_t unseen) {
    ids.resize(n);
    for (uint64_t t = 0; t < n; ++t) {
        auto it = plan->dict.find(q_sym[t]);
        ids[t] = (uint16_t)(it != plan->dict.end() ? it->second : unseen);
    }
}

// nmz_ed_plan_query_knn on a wide plan: each query's match table over the store's alphabet (one more row for symbols
// the store has never seen), then k_ed_wide_query over (query, stored trace) waves; tables in batches of <= 2 GiB
static int ed_query_wide(nmz_ed_plan *plan, const uint64_t *q_off, const uint64_t *q_sym, uint32_t n_queries,
                         uint32_t k, uint64_t *d_knn) {
    hipStream_t st = plan->ctx->stream;
    const uint32_t N = plan->n, ns1 = plan->n_sym + 1, ndw = plan->ndw;
    const uint64_t tbl = (uint64_t)ns1 * ndw;  // dwords per query table
    const uint32_t batch = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(n_queries, (2ULL << 30) / (tbl * 4)));
    uint64_t maxq = 0;
    for (uint32_t q = 0; q < n_queries; ++q)
        maxq = std::max<uint64_t>(maxq, std::min<uint64_t>(q_off[q + 1] - q_off[q], plan->maxlen));
    uint32_t *d_tbl, *d_qlen;
    uint16_t *d_ids;
    uint64_t *d_qoff;
    ScratchLayout lay;
    lay.add(&d_tbl, batch * tbl).add(&d_ids, batch * maxq + 64).add(&d_qoff, batch + 1).add(&d_qlen, batch);
    NMZ_TRY(lay.bind(plan->ctx->buf[SLOT_ED_QUERY_FORM]));
    // queries [q0, q0 + nb), each within the tables
    auto run = [&](uint32_t q0, uint32_t nb) -> int {
        const uint64_t b0 = q_off[q0], nsym = q_off[q0 + nb] - b0;
        std::vector<uint16_t> ids;
        std::vector<uint64_t> qo(nb + 1);
        std::vector<uint32_t> ql(nb);
        query_ids(plan, q_sym + b0, nsym, ids, (uint16_t)plan->n_sym);  // unseen: the spare row
        for (uint32_t q = 0; q <= nb; ++q) qo[q] = q_off[q0 + q] - b0;
        for (uint32_t q = 0; q < nb; ++q) ql[q] = (uint32_t)(qo[q + 1] - qo[q]);
        NMZ_TRY(copy_h2d(d_ids, ids.data(), nsym, st));
        NMZ_TRY(copy_h2d(d_qoff, qo.data(), nb + 1, st));
        NMZ_TRY(copy_h2d(d_qlen, ql.data(), nb, st));
        NMZ_TRY(ed_wide_build_peq(d_ids, d_qoff, nb, ns1, ndw, plan->ww, d_tbl, st));
        EdWideArgs A = ed_wide_plan_args(plan, k);
        A.peq = nullptr;  // the queries' own tables (d_tbl), one more row than the store's alphabet
        A.n_sym = ns1;
        A.knn = d_knn + (uint64_t)q0 * k;
        A.n_pairs = (uint64_t)nb * N;
        A.n_waves = A.n_pairs;
        KernelTimer kt(plan->ctx, st, "ed_wide_query");
        NMZ_TRY(ed_wide_query_launch(A, plan->ww, d_tbl, tbl, d_qlen, nb, st));
        NMZ_HIP(hipStreamSynchronize(st));  // the host vectors are pageable and the tables are reused
        return NMZ_OK;
    };
    uint32_t q0 = 0;
    for (uint32_t q = 0; q <= n_queries; ++q) {
        const bool end = q == n_queries, longq = !end && q_off[q + 1] - q_off[q] > plan->maxlen;
        if ((end || longq || q - q0 == batch) && q > q0) NMZ_TRY(run(q0, q - q0));
        if (longq) {  // longer than the tables: the generic kernel over the plan's dense ids (unseen: 0xffff)
            std::vector<uint16_t> ids;
            const uint64_t n = q_off[q + 1] - q_off[q];
            query_ids(plan, q_sym + q_off[q], n, ids, 0xffff);
            DevBuf one;
            ScopedRelease rel{one};
            uint16_t *d_one;
            ScratchLayout one_lay;
            NMZ_TRY(one_lay.add(&d_one, n + 1).bind(one));
            NMZ_TRY(copy_h2d(d_one, ids.data(), n, st));
            NMZ_TRY(ed_query_generic_launch(plan, plan->d_qoff, nullptr, plan->d_qsym, false, d_one,
                                            std::vector<uint64_t>{0}, std::vector<uint32_t>{(uint32_t)n},
                                            d_knn + (uint64_t)q * k, k));
        }
        if (end || longq || q - q0 == batch) q0 = longq ? q + 1 : q;
    }
    return NMZ_OK;
}

// nmz_ed_plan_query_knn on the other plans (k_ed_tile's dense ids, or the generic plan's u64 symbols)
static int ed_query_generic(nmz_ed_plan *plan, const uint64_t *q_off, const uint64_t *q_sym, uint32_t n_queries,
                            uint32_t k, uint64_t *d_knn) {
    hipStream_t st = plan->ctx->stream;
    const bool dense = plan->tile;  // dense u16 ids (unseen query symbols: 0xffff, never a stored id)
    static_assert(MAX_FAST_SYMBOLS <= 0xffff, "0xffff must not be a dense id");
    const uint64_t total = q_off[n_queries];
    // the queries' symbols: the one field is u16 ids on a dense plan, the u64 symbols themselves otherwise
    uint16_t *d_ids = nullptr;
    uint64_t *d_sym = nullptr;
    ScratchLayout lay;
    if (dense) lay.add(&d_ids, total + 1);
    else lay.add(&d_sym, total + 1);
    NMZ_TRY(lay.bind(plan->ctx->buf[SLOT_ED_QUERY_FORM]));
    const void *d_qs = dense ? (const void *)d_ids : (const void *)d_sym;
    std::vector<uint16_t> ids;
    if (dense) {
        query_ids(plan, q_sym, total, ids, 0xffff);
        NMZ_TRY(copy_h2d(d_ids, ids.data(), total, st));
    } else {
        NMZ_TRY(copy_h2d(d_sym, q_sym, total, st));
    }
    std::vector<uint64_t> qstart(n_queries);
    std::vector<uint32_t> qlen(n_queries);
    for (uint32_t q = 0; q < n_queries; ++q) {
        qstart[q] = q_off[q];
        qlen[q] = (uint32_t)(q_off[q + 1] - q_off[q]);
    }
    return ed_query_generic_launch(plan, dense ? plan->d_qoff : plan->d_off64,
                                   nullptr, dense ? (const void *)plan->d_qsym : (const void *)plan->d_sym64, !dense,
                                   d_qs, qstart, qlen, d_knn, k);
}

}  // namespace nmz

using namespace nmz;

extern "C" {

int nmz_ed_plan_query_knn(nmz_ed_plan *plan, const uint64_t *q_off, const uint64_t *q_sym, uint32_t n_queries,
                          uint32_t k, uint32_t *knn_id, uint32_t *knn_dist) {
    NMZ_CHECK(plan != nullptr, "plan is NULL");
    NMZ_CHECK(k >= 1 && k <= 64, "k must be in [1, 64]");
    NMZ_CHECK(n_queries == 0 || (q_off && knn_id && knn_dist), "NULL argument");
    CtxGuard g(plan->ctx);
    NMZ_TRY(g.rc);
    if (n_queries == 0) return NMZ_OK;
    const uint64_t total = q_off[n_queries];
    NMZ_CHECK(total == 0 || q_sym, "q_sym is NULL");
    for (uint32_t q = 0; q < n_queries; ++q) NMZ_CHECK(q_off[q] <= q_off[q + 1], "query offsets must not decrease");
    hipStream_t st = plan->ctx->stream;
    HostCall call(plan->ctx);
    const uint32_t N = plan->n;
    const uint64_t nk = (uint64_t)n_queries * k;
    uint64_t *d_knn;
    uint32_t *d_id, *d_ds;
    ScratchLayout lay;
    lay.add(&d_knn, nk).add(&d_id, nk).add(&d_ds, nk);
    NMZ_TRY(lay.bind(plan->ctx->buf[SLOT_KNN_LISTS_OR_TRACE_RINGS]));
    knn_init_launch(d_knn, nk, st);
    if (N) {
        if (plan->bv) NMZ_TRY(ed_query_bv(plan, q_off, q_sym, n_queries, k, d_knn));
        else if (plan->wide) NMZ_TRY(ed_query_wide(plan, q_off, q_sym, n_queries, k, d_knn));
        else NMZ_TRY(ed_query_generic(plan, q_off, q_sym, n_queries, k, d_knn));
    }
    // the query kernels list in-band results only: every other stored trace is at band + 1
    knn_fill_launch(d_knn, n_queries, k, N, plan->band + 1, 0, st);
    return knn_final_to_host(call, d_knn, nk, d_id, d_ds, knn_id, knn_dist);
}

}  // extern "C"
