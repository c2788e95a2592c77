// K9 -- move profiles: which events move between the runs of many pairs, tallied per event symbol
// (historystorage/historystorage.go:50-51 is the search interface this extends, naive/naive.go:235-257 the
// reference's equality search, naive.go:199-213 the labels that make "failing against its nearest passing run").
//
// Input: K8's output, dist[P] and ops[P][band] (ed_align.hip), over the same CSR and pairs. For a script (dist <=
// band) the r-th DEL naming value v and the r-th INS naming v are partners, a move of v: later when the INS slot
// follows the DEL slot, span = |b_pos(INS) - b_pos(DEL)|; the other DELs are dropped, the other INSs extra, a SUB
// names a[a_pos] (from) and b[b_pos] (to). Per table symbol one nmz_move_counts ("Move
// profiles").
//
// k_script_moves<LDS>: workgroups of 4 waves, one wave per pair, grid-striding over the
// pairs; the waves of a workgroup share nothing but the staged table. band <= 64, so lane s owns slot s:
//   1. the lane loads its op and, behind bounds checks, the one or two symbols it names;
//   2. one loop over the script's dist slots: the slot index is wave-uniform, so slot t's kind and names are
//      broadcast with v_readlane (no LDS); the lane counts the equal (kind, value) ops in lower lanes -- its rank --
//      and learns whether a lower lane names either of its values (the first lane naming a value counts n_pairs);
//   3. if the script has both DELs and INSs, a second loop of the same kind finds the slot with (opposite kind,
//      value, rank): the partner;
//   4. the names are looked up in usym by binary search -- in LDS when the table has at most MV_LDS_SYMS entries,
//      staged once per workgroup -- and the counters take integer atomicAdds (sums: order does not matter, the
//      result is deterministic). partner goes out with plain stores; info is summed per wave over all its pairs,
//      then per workgroup in LDS, and takes at most four atomics per workgroup at the end. No scratch, nothing
//      allocated per launch.
#include <algorithm>
#include <map>
#include <set>
#include <string>
#include <vector>

#include "ed_plan.h"
#include "nmz_common.h"
#include "nmz_internal.h"

namespace nmz {

constexpr uint32_t MV_WAVES = 4;                  // pairs in flight per workgroup
constexpr uint32_t MV_THREADS = 64 * MV_WAVES;
constexpr uint32_t MV_BLOCKS_PER_CU = 8;          // 8 waves per SIMD
static_assert(NMZ_ALIGN_MAX_BAND == 64, "a pair's ops fit one wave: one slot per lane");
static_assert(sizeof(nmz_move_counts) == 48 && sizeof(nmz_move_info) == 32, "the ABI's record sizes");

// lane t's value, t wave-uniform: two v_readlane, no LDS
__device__ __forceinline__ uint64_t mv_lane64(uint64_t v, uint32_t t) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, (int)t);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), (int)t);
    return ((uint64_t)hi << 32) | lo;
}

template <bool LDS>
__global__ __launch_bounds__(MV_THREADS) void k_script_moves(const MvArgs g) {
    __shared__ uint64_t s_tab[LDS ? MV_LDS_SYMS : 1];
    __shared__ unsigned long long s_info[4];  // the workgroup's n_scripts, n_beyond, n_ops, n_unknown
    if (threadIdx.x < 4) s_info[threadIdx.x] = 0;
    if (LDS)
        for (uint64_t i = threadIdx.x; i < g.n_usym; i += MV_THREADS) s_tab[i] = g.usym[i];
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wv = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint32_t band = g.band;
    uint64_t n_scripts = 0, n_beyond = 0, n_ops = 0, n_unknown = 0;  // wave-uniform, over the wave's pairs

    for (uint64_t p = (uint64_t)blockIdx.x * MV_WAVES + wv; p < g.n_pairs; p += (uint64_t)gridDim.x * MV_WAVES) {
        const uint32_t d = (uint32_t)__builtin_amdgcn_readfirstlane((int)g.dist[p]);
        uint32_t pr = NMZ_NONE;
        if (d > band) {
            ++n_beyond;
        } else {
            ++n_scripts;
            n_ops += d;
        }
        if (d >= 1 && d <= band) {
            const uint32_t ia = g.pairs[2 * p], ib = g.pairs[2 * p + 1];
            const uint64_t alo = g.off[ia], ahi = g.off[ia + 1], blo = g.off[ib], bhi = g.off[ib + 1];
            const uint64_t n = ahi > alo ? ahi - alo : 0, m = bhi > blo ? bhi - blo : 0;
            uint32_t kind = NMZ_NONE, ap = 0, bp = 0;
            if (lane < d) {
                const nmz_edit_op *__restrict__ o = g.ops + p * band + lane;
                ap = o->a_pos;
                bp = o->b_pos;
                kind = o->kind;
            }
            if (kind > NMZ_EDIT_INS) kind = NMZ_NONE;
            bool hasA = kind == NMZ_EDIT_SUB || kind == NMZ_EDIT_DEL;
            bool hasB = kind == NMZ_EDIT_SUB || kind == NMZ_EDIT_INS;
            if ((hasA && ap >= n) || (hasB && bp >= m)) {  // a position outside its trace: the op counts for nothing
                kind = NMZ_NONE;
                hasA = hasB = false;
            }
            const uint64_t va = hasA ? g.sym[alo + ap] : 0, vb = hasB ? g.sym[blo + bp] : 0;

            // ---- rank among equal (kind, value) ops in lower lanes; does a lower lane name va / vb?
            uint32_t rank = 0;
            bool seenA = false, seenB = false;
            for (uint32_t t = 0; t < d; ++t) {
                const uint32_t kt = (uint32_t)__builtin_amdgcn_readlane((int)kind, (int)t);
                if (kt == NMZ_NONE) continue;
                const bool below = t < lane;
                if (kt != NMZ_EDIT_INS) {  // slot t names a[a_pos]
                    const uint64_t at = mv_lane64(va, t);
                    const bool eA = hasA && at == va, eB = hasB && at == vb;
                    seenA = seenA || (below && eA);
                    seenB = seenB || (below && eB);
                    if (kt == NMZ_EDIT_DEL && kind == NMZ_EDIT_DEL && below && eA) ++rank;
                }
                if (kt != NMZ_EDIT_DEL) {  // slot t names b[b_pos]
                    const uint64_t bt = mv_lane64(vb, t);
                    const bool eA = hasA && bt == va, eB = hasB && bt == vb;
                    seenA = seenA || (below && eA);
                    seenB = seenB || (below && eB);
                    if (kt == NMZ_EDIT_INS && kind == NMZ_EDIT_INS && below && eB) ++rank;
                }
            }
            // ---- the partner: (opposite kind, value, rank)
            if (__ballot(kind == NMZ_EDIT_DEL) != 0 && __ballot(kind == NMZ_EDIT_INS) != 0) {
                for (uint32_t t = 0; t < d; ++t) {
                    const uint32_t kt = (uint32_t)__builtin_amdgcn_readlane((int)kind, (int)t);
                    if (kt != NMZ_EDIT_DEL && kt != NMZ_EDIT_INS) continue;
                    const uint32_t rt = (uint32_t)__builtin_amdgcn_readlane((int)rank, (int)t);
                    if (kt == NMZ_EDIT_DEL) {
                        const uint64_t at = mv_lane64(va, t);
                        if (kind == NMZ_EDIT_INS && vb == at && rank == rt) pr = t;
                    } else {
                        const uint64_t bt = mv_lane64(vb, t);
                        if (kind == NMZ_EDIT_DEL && va == bt && rank == rt) pr = t;
                    }
                }
            }
            const uint32_t pb = (uint32_t)__shfl((int)bp, (int)(pr != NMZ_NONE ? pr : lane));  // the partner's b_pos
            // ---- the tally
            const uint64_t iA = hasA ? (LDS ? mv_find(s_tab, g.n_usym, va) : mv_find(g.usym, g.n_usym, va)) : MV_MISS;
            const uint64_t iB = hasB ? (LDS ? mv_find(s_tab, g.n_usym, vb) : mv_find(g.usym, g.n_usym, vb)) : MV_MISS;
            n_unknown += (uint64_t)__popcll(__ballot(hasA && iA == MV_MISS));
            n_unknown += (uint64_t)__popcll(__ballot(hasB && iB == MV_MISS));
            if (iA != MV_MISS) {
                nmz_move_counts *c = g.counts + iA;
                if (kind == NMZ_EDIT_SUB) {
                    atomicAdd(&c->sub_from, 1u);
                } else if (pr == NMZ_NONE) {
                    atomicAdd(&c->dropped, 1u);
                } else {  // the DEL lane counts the move
                    const unsigned long long span = pb > bp ? pb - bp : bp - pb;
                    if (pr > lane) {
                        atomicAdd(&c->later, 1u);
                        atomicAdd((unsigned long long *)&c->span_later, span);
                    } else {
                        atomicAdd(&c->earlier, 1u);
                        atomicAdd((unsigned long long *)&c->span_earlier, span);
                    }
                }
                if (!seenA) atomicAdd(&c->n_pairs, 1u);
            }
            if (iB != MV_MISS) {
                nmz_move_counts *c = g.counts + iB;
                if (kind == NMZ_EDIT_SUB) {
                    atomicAdd(&c->sub_to, 1u);
                } else if (pr == NMZ_NONE) {
                    atomicAdd(&c->extra, 1u);
                }
                if (!seenB && !(hasA && va == vb)) atomicAdd(&c->n_pairs, 1u);
            }
        }
        if (g.partner && lane < band) g.partner[p * band + lane] = pr;
    }
    // info: the waves' sums meet in LDS, and the workgroup adds each nonzero word once (every wave's global atomics
    // on these four words serialise: measured)
    if (lane == 0) {
        if (n_scripts) atomicAdd(&s_info[0], (unsigned long long)n_scripts);
        if (n_beyond) atomicAdd(&s_info[1], (unsigned long long)n_beyond);
        if (n_ops) atomicAdd(&s_info[2], (unsigned long long)n_ops);
        if (n_unknown) atomicAdd(&s_info[3], (unsigned long long)n_unknown);
    }
    __syncthreads();
    if (threadIdx.x < 4 && s_info[threadIdx.x])
        atomicAdd((unsigned long long *)g.info + threadIdx.x, s_info[threadIdx.x]);
}

// ---- the host side ------------------------------------------------------------------------------------------------

// one live op against its traces
int moves_op_check(const nmz_edit_op &o, uint64_t n, uint64_t m, const std::string &where) {
    NMZ_CHECK(o.kind <= NMZ_EDIT_INS, "op kind " + std::to_string(o.kind) + " is not SUB, DEL or INS (" + where + ")");
    NMZ_CHECK(o.kind == NMZ_EDIT_INS || o.a_pos < n,
              "a_pos " + std::to_string(o.a_pos) + " is outside a trace of " + std::to_string(n) + " elements (" + where +
                  ")");
    NMZ_CHECK(o.kind == NMZ_EDIT_DEL || o.b_pos < m,
              "b_pos " + std::to_string(o.b_pos) + " is outside a trace of " + std::to_string(m) + " elements (" + where +
                  ")");
    return NMZ_OK;
}

// every limit of the host-pointer profile forms, no device. ops == nullptr with want_ops == false: the scripts are
// made on the device (nmz_ed_diff_profile)
int moves_validate(MvBandCheck band_ok, MvAlignValidate validate, const uint64_t *off, const uint64_t *sym,
                   uint32_t n_traces, const uint32_t *pairs, uint64_t n_pairs, uint32_t band, const uint32_t *dist,
                   const nmz_edit_op *ops, bool want_ops, const uint64_t *usym, uint64_t n_usym,
                   const nmz_move_counts *counts, const nmz_move_info *info, uint64_t *max_len) {
    // nmz_ed_diff_profile* has no ops and an optional dist: the validator only asks whether they are there
    const uint32_t some_dist = 0;
    const nmz_edit_op some_op{};
    NMZ_TRY(band_ok(band));
    NMZ_CHECK(n_pairs * (uint64_t)band < (1ull << 32) && (band == 0 || n_pairs < (1ull << 32)),
              "n_pairs * band = " + std::to_string(n_pairs) + " * " + std::to_string(band) + " must stay below 2^32: a "
              "uint32 counter could wrap");
    NMZ_TRY(validate(off, sym, n_traces, pairs, n_pairs, band, want_ops || dist ? dist : &some_dist,
                     want_ops ? ops : &some_op, max_len));
    NMZ_CHECK(n_usym == 0 || (usym && counts), "usym or counts is NULL");
    NMZ_CHECK(info != nullptr, "info is NULL");
    for (uint64_t u = 1; u < n_usym; ++u)
        NMZ_CHECK(usym[u - 1] < usym[u], "usym must be strictly increasing (entry " + std::to_string(u) + ")");
    if (!want_ops) return NMZ_OK;
    for (uint64_t p = 0; p < n_pairs; ++p) {
        if (dist[p] > band) continue;
        const uint32_t ia = pairs[2 * p], ib = pairs[2 * p + 1];
        const uint64_t n = off[ia + 1] - off[ia], m = off[ib + 1] - off[ib];
        for (uint32_t s = 0; s < dist[p]; ++s)
            NMZ_TRY(moves_op_check(ops[p * band + s], n, m,
                                   "pair " + std::to_string(p) + ", slot " + std::to_string(s)));
    }
    return NMZ_OK;
}

// partner[n_ops] by the definition: per value the queue of its DEL slots and the queue of its INS slots, in script
// order; the r-th of one is the partner of the r-th of the other. The ops are live and inside their traces.
void moves_partners(const uint64_t *a, const uint64_t *b, const nmz_edit_op *ops, uint32_t n_ops, uint32_t *partner) {
    std::map<uint64_t, std::vector<uint32_t>> dels, inss;
    for (uint32_t s = 0; s < n_ops; ++s) {
        partner[s] = NMZ_NONE;
        if (ops[s].kind == NMZ_EDIT_DEL) dels[a[ops[s].a_pos]].push_back(s);
        if (ops[s].kind == NMZ_EDIT_INS) inss[b[ops[s].b_pos]].push_back(s);
    }
    for (const auto &kv : dels) {
        auto it = inss.find(kv.first);
        if (it == inss.end()) continue;
        for (size_t r = 0; r < std::min(kv.second.size(), it->second.size()); ++r) {
            partner[kv.second[r]] = it->second[r];
            partner[it->second[r]] = kv.second[r];
        }
    }
}

int moves_enqueue(nmz_ctx *ctx, hipStream_t st, const MvArgs &a, int accumulate) {
    NMZ_TRY(align_band(a.band));
    NMZ_CHECK(a.n_pairs * (uint64_t)a.band < (1ull << 32) && (a.band == 0 || a.n_pairs < (1ull << 32)),
              "n_pairs * band = " + std::to_string(a.n_pairs) + " * " + std::to_string(a.band) + " must stay below "
              "2^32: a uint32 counter could wrap");
    NMZ_CHECK(a.n_usym == 0 || (a.usym && a.counts), "d_usym or d_counts is NULL");
    NMZ_CHECK(a.info != nullptr, "d_info is NULL");
    NMZ_CHECK(a.n_usym <= SIZE_MAX / sizeof(nmz_move_counts), "n_usym does not fit the counters");
    if (!accumulate) {
        if (a.n_usym) NMZ_HIP(hipMemsetAsync(a.counts, 0, (size_t)a.n_usym * sizeof(nmz_move_counts), st));
        NMZ_HIP(hipMemsetAsync(a.info, 0, sizeof(nmz_move_info), st));
    }
    if (a.n_pairs == 0) return NMZ_OK;
    NMZ_CHECK(a.off && a.pairs && a.dist, "d_off, d_pairs or d_dist is NULL");
    NMZ_CHECK(a.band == 0 || a.ops, "d_ops is NULL");
    const unsigned blocks = (unsigned)std::min<uint64_t>((a.n_pairs + MV_WAVES - 1) / MV_WAVES,
                                                         (uint64_t)std::max(ctx->n_cu, 1) * MV_BLOCKS_PER_CU);
    KernelTimer kt(ctx, st, "script_moves");
    if (a.n_usym <= MV_LDS_SYMS)
        hipLaunchKernelGGL(k_script_moves<true>, dim3(blocks), dim3(MV_THREADS), 0, st, a);
    else
        hipLaunchKernelGGL(k_script_moves<false>, dim3(blocks), dim3(MV_THREADS), 0, st, a);
    if (hipGetLastError() != hipSuccess) return fail(NMZ_EHIP, "k_script_moves launch failed");
    return NMZ_OK;
}

void moves_zero(nmz_move_counts *counts, uint64_t n_usym, nmz_move_info *info) {
    for (uint64_t u = 0; u < n_usym; ++u) counts[u] = nmz_move_counts{};
    *info = nmz_move_info{};
}

// the profile by the definition, for any band the validator lets through: plain loops, a set of the names per
// script, std::lower_bound into the table. Nothing shared with the kernels.
int moves_profile_host(MvBandCheck band_ok, MvAlignValidate validate, const uint64_t *off, const uint64_t *sym,
                       uint32_t n_traces, const uint32_t *pairs, uint64_t n_pairs, uint32_t band, const uint32_t *dist,
                       const nmz_edit_op *ops, const uint64_t *usym, uint64_t n_usym, uint32_t *partner,
                       nmz_move_counts *counts, nmz_move_info *info) {
    uint64_t max_len = 0;
    NMZ_TRY(moves_validate(band_ok, validate, off, sym, n_traces, pairs, n_pairs, band, dist, ops, true, usym, n_usym,
                           counts, info, &max_len));
    moves_zero(counts, n_usym, info);
    auto find = [&](uint64_t v) -> nmz_move_counts * {
        const uint64_t *at = std::lower_bound(usym, usym + n_usym, v);
        if (at == usym + n_usym || *at != v) {
            ++info->n_unknown;
            return nullptr;
        }
        return counts + (at - usym);
    };
    std::vector<uint32_t> pr(band);
    for (uint64_t p = 0; p < n_pairs; ++p) {
        uint32_t *out = partner ? partner + p * band : nullptr;
        for (uint32_t s = 0; out && s < band; ++s) out[s] = NMZ_NONE;
        if (dist[p] > band) {
            ++info->n_beyond;
            continue;
        }
        ++info->n_scripts;
        info->n_ops += dist[p];
        const uint64_t *a = sym + off[pairs[2 * p]], *b = sym + off[pairs[2 * p + 1]];
        const nmz_edit_op *o = ops + p * band;
        moves_partners(a, b, o, dist[p], pr.data());
        std::set<uint64_t> named;
        for (uint32_t s = 0; s < dist[p]; ++s) {
            if (out) out[s] = pr[s];
            if (o[s].kind == NMZ_EDIT_SUB) {
                named.insert(a[o[s].a_pos]);
                named.insert(b[o[s].b_pos]);
                if (nmz_move_counts *c = find(a[o[s].a_pos])) ++c->sub_from;
                if (nmz_move_counts *c = find(b[o[s].b_pos])) ++c->sub_to;
            } else if (o[s].kind == NMZ_EDIT_DEL) {
                named.insert(a[o[s].a_pos]);
                nmz_move_counts *c = find(a[o[s].a_pos]);
                if (!c) continue;
                if (pr[s] == NMZ_NONE) {
                    ++c->dropped;
                    continue;
                }
                const uint32_t bi = o[pr[s]].b_pos, bd = o[s].b_pos;
                const uint64_t span = bi > bd ? bi - bd : bd - bi;
                if (pr[s] > s) {
                    ++c->later;
                    c->span_later += span;
                } else {
                    ++c->earlier;
                    c->span_earlier += span;
                }
            } else {
                named.insert(b[o[s].b_pos]);
                nmz_move_counts *c = find(b[o[s].b_pos]);  // a partnered INS: its DEL counts the move
                if (c && pr[s] == NMZ_NONE) ++c->extra;
            }
        }
        for (uint64_t v : named) {
            const uint64_t *at = std::lower_bound(usym, usym + n_usym, v);
            if (at != usym + n_usym && *at == v) ++counts[at - usym].n_pairs;
        }
    }
    return NMZ_OK;
}

}  // namespace nmz

using namespace nmz;

extern "C" {

// One script on the calling thread (historystorage.go:50-51, naive.go:235-257): the definition, nothing shared with
// the kernel.
int nmz_script_moves_host(const uint64_t *a, uint64_t n, const uint64_t *b, uint64_t m, const nmz_edit_op *ops,
                          uint32_t n_ops, uint32_t *partner) {
    NMZ_CHECK((n == 0 || a) && (m == 0 || b), "a or b is NULL");
    NMZ_CHECK(n_ops == 0 || (ops && partner), "ops or partner is NULL");
    for (uint32_t s = 0; s < n_ops; ++s) NMZ_TRY(moves_op_check(ops[s], n, m, "slot " + std::to_string(s)));
    moves_partners(a, b, ops, n_ops, partner);
    return NMZ_OK;
}

// The whole profile on the calling thread (historystorage.go:50-51, naive.go:199-213, 235-257): plain loops, a set
// of the names per script, std::lower_bound into the table.
int nmz_move_profile_host(const uint64_t *off, const uint64_t *sym, uint32_t n_traces, const uint32_t *pairs,
                          uint64_t n_pairs, uint32_t band, const uint32_t *dist, const nmz_edit_op *ops,
                          const uint64_t *usym, uint64_t n_usym, uint32_t *partner, nmz_move_counts *counts,
                          nmz_move_info *info) {
    return moves_profile_host(align_band, align_validate, off, sym, n_traces, pairs, n_pairs, band, dist, ops, usym,
                              n_usym, partner, counts, info);
}

int nmz_move_profile_dev(nmz_ctx *ctx, const uint64_t *d_off, const uint64_t *d_sym, const uint32_t *d_pairs,
                         uint64_t n_pairs, uint32_t band, const uint32_t *d_dist, const nmz_edit_op *d_ops,
                         const uint64_t *d_usym, uint64_t n_usym, uint32_t *d_partner, nmz_move_counts *d_counts,
                         nmz_move_info *d_info, int accumulate, void *stream) {
    NMZ_CHECK(ctx != nullptr, "ctx is NULL");
    CtxGuard g(ctx);
    NMZ_TRY(g.rc);
    const MvArgs a{d_off, d_sym, d_pairs, n_pairs, band, d_dist, d_ops, d_usym, n_usym, d_partner, d_counts, d_info};
    return moves_enqueue(ctx, stream ? (hipStream_t)stream : ctx->stream, a, accumulate);
}

int nmz_move_profile(nmz_ctx *ctx, const uint64_t *off, const uint64_t *sym, uint32_t n_traces, const uint32_t *pairs,
                     uint64_t n_pairs, uint32_t band, const uint32_t *dist, const nmz_edit_op *ops,
                     const uint64_t *usym, uint64_t n_usym, uint32_t *partner, nmz_move_counts *counts,
                     nmz_move_info *info) {
    // the arguments first: they are checked without a device
    uint64_t max_len = 0;
    NMZ_TRY(moves_validate(align_band, align_validate, off, sym, n_traces, pairs, n_pairs, band, dist, ops, true, usym,
                           n_usym, counts, info, &max_len));
    if (n_pairs == 0) {  // all zero: no device either
        moves_zero(counts, n_usym, info);
        return NMZ_OK;
    }
    NMZ_CHECK(ctx != nullptr, "ctx is NULL");
    CtxGuard g(ctx);
    NMZ_TRY(g.rc);
    HostCall call(ctx);  // owns no plan: call.work holds the buffers, drained before they go back to the pool
    hipStream_t st = ctx->stream;
    const uint64_t total = off[n_traces];
    const size_t n_slots = (size_t)n_pairs * band;
    uint64_t *d_off, *d_sym, *d_usym;
    uint32_t *d_pairs, *d_dist, *d_partner;
    nmz_edit_op *d_ops;
    nmz_move_counts *d_counts;
    nmz_move_info *d_info;
    ScratchLayout lay;
    lay.add(&d_off, n_traces + 1).add(&d_sym, total + 1).add(&d_pairs, 2 * n_pairs).add(&d_dist, n_pairs);
    lay.add(&d_ops, n_slots + 1).add(&d_usym, n_usym + 1).add(&d_partner, n_slots + 1).add(&d_counts, n_usym + 1);
    lay.add(&d_info, 1);
    NMZ_TRY(lay.bind(call.work));
    NMZ_TRY(upload_csr(d_off, d_sym, off, sym, n_traces, st));
    NMZ_TRY(copy_h2d(d_pairs, pairs, 2 * n_pairs, st));
    NMZ_TRY(copy_h2d(d_dist, dist, n_pairs, st));
    NMZ_TRY(copy_h2d(d_ops, ops, n_slots, st));
    NMZ_TRY(copy_h2d(d_usym, usym, n_usym, st));
    const MvArgs a{d_off, d_sym, d_pairs, n_pairs, band, d_dist, d_ops, d_usym, n_usym, partner ? d_partner : nullptr,
                   d_counts, d_info};
    NMZ_TRY(moves_enqueue(ctx, st, a, 0));
    if (partner) NMZ_TRY(copy_d2h(partner, d_partner, n_slots, st));
    NMZ_TRY(copy_d2h(counts, d_counts, n_usym, st));
    NMZ_TRY(copy_d2h(info, d_info, 1, st));
    return call.done();
}

int nmz_ed_diff_profile(nmz_ctx *ctx, const uint64_t *off, const uint64_t *sym, uint32_t n_traces,
                        const uint32_t *pairs, uint64_t n_pairs, uint32_t band, const uint64_t *usym, uint64_t n_usym,
                        uint32_t *dist, nmz_move_counts *counts, nmz_move_info *info) {
    // the arguments first: they are checked without a device
    uint64_t max_len = 0, slot_words = 0;
    NMZ_TRY(moves_validate(align_band, align_validate, off, sym, n_traces, pairs, n_pairs, band, dist, nullptr, false,
                           usym, n_usym, counts, info, &max_len));
    if (n_pairs == 0) {  // all zero: no device either
        moves_zero(counts, n_usym, info);
        return NMZ_OK;
    }
    NMZ_TRY(align_shape(band, max_len, &slot_words));
    NMZ_CHECK(ctx != nullptr, "ctx is NULL");
    CtxGuard g(ctx);
    NMZ_TRY(g.rc);
    HostCall call(ctx);
    nmz_ed_align_plan *plan = nullptr;
    NMZ_TRY(align_plan_create_locked(ctx, band, max_len, slot_words, &plan));
    call.own_plan<align_plan_destroy_locked>(plan);
    hipStream_t st = ctx->stream;
    const uint64_t total = off[n_traces];
    const size_t n_slots = (size_t)n_pairs * band;
    uint64_t *d_off, *d_sym, *d_usym;
    uint32_t *d_pairs, *d_dist;
    nmz_edit_op *d_ops;
    nmz_move_counts *d_counts;
    nmz_move_info *d_info;
    ScratchLayout lay;
    lay.add(&d_off, n_traces + 1).add(&d_sym, total + 1).add(&d_pairs, 2 * n_pairs).add(&d_dist, n_pairs);
    lay.add(&d_ops, n_slots + 1).add(&d_usym, n_usym + 1).add(&d_counts, n_usym + 1).add(&d_info, 1);
    NMZ_TRY(lay.bind(call.work));
    NMZ_TRY(upload_csr(d_off, d_sym, off, sym, n_traces, st));
    NMZ_TRY(copy_h2d(d_pairs, pairs, 2 * n_pairs, st));
    NMZ_TRY(copy_h2d(d_usym, usym, n_usym, st));
    NMZ_TRY(align_enqueue(plan, st, d_off, d_sym, d_pairs, n_pairs, d_dist, d_ops));
    const MvArgs a{d_off, d_sym, d_pairs, n_pairs, band, d_dist, d_ops, d_usym, n_usym, nullptr, d_counts, d_info};
    NMZ_TRY(moves_enqueue(ctx, st, a, 0));
    if (dist) NMZ_TRY(copy_d2h(dist, d_dist, n_pairs, st));
    NMZ_TRY(copy_d2h(counts, d_counts, n_usym, st));
    NMZ_TRY(copy_d2h(info, d_info, 1, st));
    return call.done();
}

}  // extern "C"
