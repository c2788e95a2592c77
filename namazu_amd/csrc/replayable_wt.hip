// K1 -- replayable-policy seed sweep statistics from wavelet trees (replayablepolicy.go:100-114).
//
// What a sweep returns per seed is the statistics of its E decisions t_e = FNV1a64(seed || hint_e) % m:
// the sum, the maximum and the first event index of the maximum. replayable.hip explains the algebra this
// starts from: per (table row L, hint-length class) segment of n events, sorted by the FNV correction C,
//     t_i = (b_i + Cm_i) mod m,   b_i = Hm for i < d (carry-free prefix), Hm2 for i >= d,
// where d = #{C_i <= ~H} and every t wraps at most once. So per (seed, segment)
//     sum  = d Hm + (n - d) Hm2 + sum Cm - m W,   W = #{i < d: Cm_i >= m - Hm} + #{i >= d: Cm_i >= m - Hm2}
//     max  = over the two parts, b + (the largest Cm below m - b), or, when no Cm of the part is below m - b,
//            b + (the part's largest Cm) - m.
// Both are 2-D dominance queries over the points (position i, rank of (Cm_i, ~e_i)). The plan stores, per
// (row, segment), a levelwise wavelet tree over the rank permutation in position order; a query answers
// "how many of positions < d have rank >= R" in one read per level, and the same descent finds the level
// where the predecessor of R inside the part branches off, from which a short second descent reaches it.
// Ranks sort by (Cm ascending, e descending), so among equal Cm the highest rank is the first event: the
// predecessor's event is the reference's first-index argmax (the order of its `>` test).
// A plan whose row image stays small enough (configs[1]'s) stores, instead of the levels, one plane per boundary
// between 64-rank blocks: the count is then two plane reads and a mask, the predecessor a search over blocks
// (wt_plane_bytes, wt_pred_planes).
//
// Per (seed, segment of n ~ 2,000 events): ~3 lifting searches of ~5 LDS reads (d over C's high words,
// R_A and R_B over the sorted Cm through 256-bucket indexes), 2 x ceil(log2 n + 1) descent reads, a few
// predecessor reads -- ~50 LDS reads instead of ~150 for the sorted-block searches of k_replayable_sweep_oq,
// and a row image of ~13 B per event instead of ~27, so two rows fit one CU's LDS.
//
// This file is the sweep. The plan kernel that builds the row images is in replayable_wt_plan.hip, the top-k
// selection over the sweep's chunk records in replayable_wt_topk_dev.h (device code, compiled here: see there), what
// the three share in replayable_wt_dev.h.
#include <cstdlib>
#include <initializer_list>

#include "nmz_common.h"
#include "nmz_internal.h"
#include "replayable_plan.h"
#include "replayable_wt_dev.h"

namespace nmz {

// A block's prefix mask (2^BB bits) and the few operations the descents need on it
template <int BB>
struct WtMask;
template <>
struct WtMask<5> {
    using T = uint32_t;
    static __device__ __forceinline__ T load(const char *mk, uint32_t i) {
        return reinterpret_cast<const uint32_t *>(mk)[i];
    }
    static __device__ __forceinline__ uint32_t count_ge(T v, uint32_t r) { return __popc(v >> r); }  // bits >= r
    static __device__ __forceinline__ T below(T v, uint32_t r) { return __builtin_amdgcn_ubfe(v, 0u, r); }  // r < 32
    static __device__ __forceinline__ T low(T v, uint32_t s) { return v & (0xffffffffu >> (32u - s)); }  // 1..32
    static __device__ __forceinline__ T inv(T v) { return ~v; }
    static __device__ __forceinline__ bool any(T v) { return v != 0; }
    static __device__ __forceinline__ uint32_t top(T v) { return 31u - __clz(v); }  // v != 0
};
template <>
struct WtMask<6> {
    using T = uint64_t;
    static __device__ __forceinline__ T load(const char *mk, uint32_t i) {
        return reinterpret_cast<const uint64_t *>(mk)[i];
    }
    static __device__ __forceinline__ uint32_t count_ge(T v, uint32_t r) { return (uint32_t)__popcll(v >> r); }
    static __device__ __forceinline__ T below(T v, uint32_t r) { return v & ((1ull << r) - 1ull); }
    static __device__ __forceinline__ T low(T v, uint32_t s) { return v & (~0ull >> (64u - s)); }
    static __device__ __forceinline__ T inv(T v) { return ~v; }
    static __device__ __forceinline__ bool any(T v) { return v != 0; }
    static __device__ __forceinline__ uint32_t top(T v) { return 63u - (uint32_t)__clzll(v); }
};
struct WtMask128 {
    uint64_t lo, hi;
};
template <>
struct WtMask<7> {
    using T = WtMask128;
    static __device__ __forceinline__ T load(const char *mk, uint32_t i) {
        const uint4 x = reinterpret_cast<const uint4 *>(mk)[i];
        return T{((uint64_t)x.y << 32) | x.x, ((uint64_t)x.w << 32) | x.z};
    }
    static __device__ __forceinline__ uint32_t count_ge(T v, uint32_t r) {
        return r < 64 ? (uint32_t)(__popcll(v.lo >> r) + __popcll(v.hi)) : (uint32_t)__popcll(v.hi >> (r - 64));
    }
    static __device__ __forceinline__ T below(T v, uint32_t r) {
        return r < 64 ? T{v.lo & ((1ull << r) - 1ull), 0ull} : T{v.lo, v.hi & ((1ull << (r - 64)) - 1ull)};
    }
    static __device__ __forceinline__ T low(T v, uint32_t s) {
        return s <= 64 ? T{v.lo & (~0ull >> (64u - s)), 0ull} : T{v.lo, v.hi & (~0ull >> (128u - s))};
    }
    static __device__ __forceinline__ T inv(T v) { return T{~v.lo, ~v.hi}; }
    static __device__ __forceinline__ bool any(T v) { return (v.lo | v.hi) != 0; }
    static __device__ __forceinline__ uint32_t top(T v) {
        return v.hi ? 127u - (uint32_t)__clzll(v.hi) : 63u - (uint32_t)__clzll(v.lo);
    }
};

// one decision from a table entry {C lo, C hi, Cm, ~e}: counts carry-free events (d) and wraps (W).
// BIG: m >= 2^31, where base + Cm can overflow 32 bits (the true sum then exceeds m and t = sum - m is exact
// modulo 2^32)
template <bool BIG>
__device__ __forceinline__ void wt_decide(uint4 q, uint64_t nH, uint32_t Hm, uint32_t Hm2, uint32_t m, uint32_t &d,
                                          uint32_t &W, uint64_t &key) {
    const bool nc = (((uint64_t)q.y << 32) | q.x) <= nH;
    const uint32_t b = nc ? Hm : Hm2;
    const uint32_t s = b + q.z;
    const bool wrap = BIG ? (s < b || s >= m) : s >= m;
    const uint32_t t = wrap ? s - m : s;
    d += nc;
    W += wrap;
    const uint64_t k = ((uint64_t)t << 32) | q.w;
    key = k > key ? k : key;
}

// Wave-uniform operands of the descents copied into VGPRs, so their VOP2 forms take no SGPR or inline-constant
// operand (tools/ubench measures those forms at half the VGPR-only issue rate): 1-2 % on K1, consistently across
// four A/B pairs (profiles/r03r_wt_vgprc_ab.json)
__device__ __forceinline__ uint32_t wt_v(uint32_t x) {
    uint32_t v;
    asm volatile("v_mov_b32 %0, %1" : "=v"(v) : "s"(x));
    return v;
}

// wave-uniform constants the sweep keeps in VGPRs (operands of VOP2 forms)
struct WtVConst {
    uint32_t st4[5];  // lifting-search steps in bytes: 4 << r
};

// the two bases of a segment: Hm = H mod m for the carry-free prefix (C <= ~H = nH), Hm2 = (H + 2^64) mod m past it
template <bool BIG, int NS>
__device__ __forceinline__ void wt_bases(const WtClass &ci, const uint64_t (&h0)[NS], uint32_t m, uint64_t mu,
                                         uint32_t m_k64, uint64_t (&nH)[NS], uint32_t (&Hm)[NS], uint32_t (&Hm2)[NS]) {
#pragma unroll
    for (int u = 0; u < NS; ++u) {
        const uint64_t H = h0[u] * ci.pn;
        nH[u] = ~H;
        Hm[u] = BIG ? mod_barrett64(H, m, mu) : mod_barrett_small(H, m, mu);
        const uint32_t t2 = Hm[u] + m_k64;
        Hm2[u] = BIG ? ((t2 < Hm[u] || t2 >= m) ? t2 - m : t2) : min(t2, t2 - m);
    }
}

// One seed's statistics over one segment: adds d Hm + (n - d) Hm2 to sum, the segment's wraps to W, and folds its
// maximum key {t, ~e} into key. Its steps, as the file header describes them: (1) the two bases; (2) a short segment:
// every decision from the table row; (3) the three lifting searches for d, R_A, R_B; (4) counts and predecessors,
// from planes or from levels; (5) the two parts' maxima folded into key.
// The steps after the first stay in one body: cut out as functions (each was tried, on its own) the blocks of every
// one of them come out in another order after inlining and the kernels' machine code changes, which would make
// the profiles recorded for these kernels stale (profiles/valu_per_unit.json).
// NS seeds per lane (arrays indexed by u, unrolled): the wave-uniform control -- segment parameters, lifting
// rounds, level constants, loop trips, ballots -- is paid once for NS seeds, and the NS seeds' read chains are
// independent, so a wave keeps 2 NS dependent LDS chains in flight per descent level instead of 2.
// PL (BB = 6 only): the plan's segments hold rank-block planes instead of levels.
template <bool BIG, int NS, int BB, bool PL>
__device__ __forceinline__ void wt_seed_class(const WtVConst &vc, const WtClass &ci, const char *__restrict__ img,
                                              const uint4 *__restrict__ row, const uint64_t (&h0)[NS], uint32_t m,
                                              uint64_t mu, uint32_t m_k64, uint32_t msh, uint64_t (&sum)[NS],
                                              uint32_t (&W)[NS], uint64_t (&key)[NS]) {
    const uint32_t n = ci.n;
    // (1) the bases
    uint64_t nH[NS];
    uint32_t Hm[NS], Hm2[NS];
    wt_bases<BIG, NS>(ci, h0, m, mu, m_k64, nH, Hm, Hm2);
    // (2) a segment without an image
    if (n <= WT_BRUTE) {
#pragma unroll
        for (int u = 0; u < NS; ++u) {
            uint32_t d = 0;
            for (uint32_t i = 0; i < n; ++i) wt_decide<BIG>(row[ci.start + i], nH[u], Hm[u], Hm2[u], m, d, W[u], key[u]);
            sum[u] += (uint64_t)d * Hm[u] + (uint64_t)(n - d) * Hm2[u];
        }
        return;
    }
    // (3) the lifting searches
    const uint32_t *__restrict__ cm = reinterpret_cast<const uint32_t *>(img + ci.o_cm);
    const uint32_t *__restrict__ chi = reinterpret_cast<const uint32_t *>(img + ci.o_chi);
    const uint16_t *__restrict__ ev = reinterpret_cast<const uint16_t *>(img + ci.o_e);
    const uint16_t *__restrict__ im = reinterpret_cast<const uint16_t *>(img + ci.o_im);
    const uint16_t *__restrict__ ic = reinterpret_cast<const uint16_t *>(img + ci.o_ic);
    uint32_t nh[NS], XA[NS], XB[NS];
    const uint32_t *pa[NS], *pb[NS], *pc[NS];
#pragma unroll
    for (int u = 0; u < NS; ++u) {
        nh[u] = (uint32_t)(nH[u] >> 32);
        XA[u] = m - Hm[u];  // t wraps <=> Cm >= X
        XB[u] = m - Hm2[u];
        // three lifting searches stepped together (every read of a round in flight at once) from the bucket starts:
        // every entry past the bucket is >= the bound, and the sentinel at n ends every probe past the array
        // (pointer form: a round's probes are LDS reads with immediate offsets; WT_PAD sentinels end the probes of up
        // to five rounds past the array, longer searches -- repeated hints -- clamp at the sentinel at n)
        pa[u] = chi + ic[nh[u] >> 24];
        pb[u] = cm + im[XA[u] >> msh];
        pc[u] = cm + im[XB[u] >> msh];
    }
    const uint32_t rS = ci.rS;
    if (rS <= 5) {
#pragma unroll
        for (int r = 4; r >= 0; --r) {
            if (rS > (uint32_t)r) {
                constexpr uint32_t one = 1;
                const uint32_t st = one << r, st4 = vc.st4[r];  // the step in bytes, in a VGPR (a VOP2 select)
#pragma unroll
                for (int u = 0; u < NS; ++u) {
                    const uint32_t a = pa[u][st - 1], b = pb[u][st - 1], c = pc[u][st - 1];
                    pa[u] = reinterpret_cast<const uint32_t *>(reinterpret_cast<const char *>(pa[u]) + (a < nh[u] ? st4 : 0u));
                    pb[u] = reinterpret_cast<const uint32_t *>(reinterpret_cast<const char *>(pb[u]) + (b < XA[u] ? st4 : 0u));
                    pc[u] = reinterpret_cast<const uint32_t *>(reinterpret_cast<const char *>(pc[u]) + (c < XB[u] ? st4 : 0u));
                }
            }
        }
    } else {
        const uint32_t *ea = chi + n, *eb = cm + n;
        for (uint32_t st = (1u << rS) >> 1; st; st >>= 1) {
#pragma unroll
            for (int u = 0; u < NS; ++u) {
                const uint32_t a = *min(pa[u] + st - 1, ea), b = *min(pb[u] + st - 1, eb), c = *min(pc[u] + st - 1, eb);
                pa[u] += a < nh[u] ? st : 0u;
                pb[u] += b < XA[u] ? st : 0u;
                pc[u] += c < XB[u] ? st : 0u;
            }
        }
    }
    // (LDS addresses: the low words of the generic pointers)
    auto lo = [](const uint32_t *q) { return (uint32_t)reinterpret_cast<uintptr_t>(q); };
    uint32_t d[NS], RA[NS], RB[NS];
#pragma unroll
    for (int u = 0; u < NS; ++u) {
        RA[u] = (lo(pb[u]) - lo(cm)) >> 2;
        RB[u] = (lo(pc[u]) - lo(cm)) >> 2;
        // d = #{C <= ~H}: #{C_hi < ~H_hi} plus the entries whose high word equals ~H_hi and low word is <= ~H_lo
        // (about n / 2^32 of the queries: the low words come from the table row)
        d[u] = (lo(pa[u]) - lo(chi)) >> 2;
        if (chi[d[u]] == nh[u]) {
            const uint32_t nl = (uint32_t)nH[u];
            while (d[u] < n && chi[d[u]] == nh[u] && row[ci.start + d[u]].x <= nl) ++d[u];
        }
    }
    const char *__restrict__ mk = img + ci.o_mk;
    using MK = WtMask<BB>;
    using MT = typename MK::T;
    constexpr uint32_t BW = 1u << BB, BM = BW - 1;
    // (4) counts (the segment's wraps, into W) and each part's maximum: the rank pA / pB of its predecessor of R, or of
    // its largest element when it wraps
    uint32_t pA[NS], pB[NS];
    bool wrapA[NS], wrapB[NS];
    if constexpr (PL) {
        // from planes: f_b(d) = #{i < d: rank_i >= 64 b} is one read of plane b (b = 0 .. NB, NB = (n >> 6) + 1), so with
        // b = R >> 6 the prefix part has o = f_b(d) - f_{b+1}(d) elements in R's block -- the index of the block's
        // prefix mask -- and f_{b+1}(d) + count_ge(mask, R & 63) ranks >= R: two dependent rounds for both counts.
        static_assert(!PL || BB == 6, "planes stand on 64-rank blocks");
        const uint32_t NB = (n >> 6) + 1;
        const uint32_t nv = wt_v(n), nw8 = wt_v(ci.nw * 8u), nbv = wt_v(NB), six = wt_v(6u);
        const char *pd[NS];  // the word of position d in plane 0; plane b's is nw8 * b bytes on
        auto fcount = [](const char *q, uint32_t dd) {
            const uint2 w = *reinterpret_cast<const uint2 *>(q);
            return w.y + __popc(__builtin_amdgcn_ubfe(w.x, 0u, dd));
        };
        uint32_t bA[NS], bB[NS], fA0[NS], fB0[NS], cA[NS], cB[NS];
        MT belA[NS], belB[NS];
        bool hitA[NS], hitB[NS];
#pragma unroll
        for (int u = 0; u < NS; ++u) {
            pd[u] = img + ci.o_pl + (d[u] >> 5) * 8u;
            bA[u] = RA[u] >> six;
            bB[u] = RB[u] >> six;
            const char *qa = pd[u] + bA[u] * nw8, *qb = pd[u] + bB[u] * nw8;
            fA0[u] = fcount(qa, d[u]);
            fB0[u] = fcount(qb, d[u]);
            const uint32_t fA1 = fcount(qa + nw8, d[u]), fB1 = fcount(qb + nw8, d[u]);
            const uint32_t rA = RA[u] & BM, rB = RB[u] & BM;
            const MT mA = MK::load(mk, (RA[u] & ~BM) + bA[u] + (fA0[u] - fA1));
            const MT mB = MK::load(mk, (RB[u] & ~BM) + bB[u] + (fB0[u] - fB1));
            cA[u] = fA1 + MK::count_ge(mA, rA);
            cB[u] = fB1 + MK::count_ge(mB, rB);
            W[u] += cA[u] + (n - RB[u]) - cB[u];
            belA[u] = MK::below(mA, rA);
            belB[u] = MK::below(MK::inv(mB), rB);
            hitA[u] = MK::any(belA[u]);
            hitB[u] = MK::any(belB[u]);
        }
        // predecessors outside R's block: a search over blocks. The suffix part's counts are
        // g_b(d) = #{i >= d: rank_i >= 64 b} = n - 64 b - f_b(d) (negative only at b = NB: compared signed). A part
        // with elements below R (d - cA of the prefix, R_B - (d - cB) of the suffix) takes the largest block of
        // [0, b - 1] whose count exceeds block b's; a part with none wraps and takes the largest block of [b, NB - 1]
        // with any element. Counts do not increase with b: one lifting search from the range's first block, reads
        // clamped to plane NB (all zeros); steps longer than every lane's range are skipped.
        constexpr uint32_t OFF = 0x7fffffffu;  // no count exceeds it: the lanes that search nothing stay at block 0
        uint32_t posA[NS], posB[NS], TA[NS], TB[NS], rng = 0;
#pragma unroll
        for (int u = 0; u < NS; ++u) {
            const bool dA = d[u] > 0 && !hitA[u], dB = d[u] < n && !hitB[u];
            wrapA[u] = dA && d[u] == cA[u];
            wrapB[u] = dB && RB[u] + cB[u] == d[u];
            posA[u] = wrapA[u] ? bA[u] : 0u;
            posB[u] = wrapB[u] ? bB[u] : 0u;
            TA[u] = !dA ? OFF : wrapA[u] ? 0u : fA0[u];
            TB[u] = !dB ? OFF : wrapB[u] ? 0u : nv - (bB[u] << six) - fB0[u];
            const uint32_t rA = !dA ? 0u : wrapA[u] ? nbv - 1u - bA[u] : bA[u] - 1u;
            const uint32_t rB = !dB ? 0u : wrapB[u] ? nbv - 1u - bB[u] : bB[u] - 1u;
            rng = max(rng, max(rA, rB));
        }
        if (__builtin_amdgcn_ballot_w64(rng != 0)) {
#pragma unroll
            for (uint32_t st = 32; st; st >>= 1) {
                if (st >= NB || !__builtin_amdgcn_ballot_w64(rng >= st)) continue;
                const uint32_t stv = wt_v(st);
#pragma unroll
                for (int u = 0; u < NS; ++u) {
                    const uint32_t qa = min(posA[u] + stv, nbv), qb = min(posB[u] + stv, nbv);
                    const uint32_t fa = fcount(pd[u] + qa * nw8, d[u]), fb = fcount(pd[u] + qb * nw8, d[u]);
                    posA[u] = (int32_t)fa > (int32_t)TA[u] ? qa : posA[u];
                    posB[u] = (int32_t)(nv - (qb << six) - fb) > (int32_t)TB[u] ? qb : posB[u];
                }
            }
        }
        // the found block's prefix count, then its mask: the prefix part's largest rank there, or the suffix part's
        // (the inverted mask cut to the block's min(n - 64 pos, 64) ranks)
#pragma unroll
        for (int u = 0; u < NS; ++u) {
            const char *qa = pd[u] + posA[u] * nw8, *qb = pd[u] + posB[u] * nw8;
            const uint32_t oa = fcount(qa, d[u]) - fcount(qa + nw8, d[u]);
            const uint32_t ob = fcount(qb, d[u]) - fcount(qb + nw8, d[u]);
            const uint32_t sa = posA[u] << six, sb = posB[u] << six;
            const MT vA = MK::load(mk, sa + posA[u] + oa);
            const MT vB = MK::low(MK::inv(MK::load(mk, sb + posB[u] + ob)), min(nv - sb, BW));
            pA[u] = hitA[u] ? (RA[u] & ~BM) + MK::top(belA[u]) : sa + MK::top(vA);
            pB[u] = hitB[u] ? (RB[u] & ~BM) + MK::top(belB[u]) : sb + MK::top(vB);
        }
    } else {
    // from levels (this arm keeps the function's indentation):
    // descents along R_A's and R_B's paths with the prefix [0, d) down to R's rank block, branch-free with every
    // read of a level in flight: counts of ranks >= R, and the deepest level where a part's elements below R branch
    // off (the predecessor's subtree: node start s, prefix offset q)
    const uint2 *__restrict__ lv = reinterpret_cast<const uint2 *>(img + ci.o_lv);
    const uint32_t K = ci.K, nw = ci.nw, lb = wt_levels(K, BB);
    uint32_t oA[NS], oB[NS], cA[NS], cB[NS], lA[NS], sA[NS], qA[NS], lB[NS], sB[NS], qB[NS];
#pragma unroll
    for (int u = 0; u < NS; ++u) {
        oA[u] = oB[u] = d[u];
        cA[u] = cB[u] = 0;
        lA[u] = lB[u] = WT_NONE;
        sA[u] = qA[u] = sB[u] = qB[u] = 0;
    }
    const uint32_t nv = wt_v(n), one = wt_v(1u), five = wt_v(5u);
    if (lb) {
        // level 0 (the root: both chains at offset d, one read); then the level constants live in VGPRs, halved per
        // level (no SGPR operands, no per-level scalar shifts)
        const uint32_t hs = 1u << (K - 1);
#pragma unroll
        for (int u = 0; u < NS; ++u) {
            const uint2 w = lv[d[u] >> 5];
            const uint32_t o = w.y + __popc(__builtin_amdgcn_ubfe(w.x, 0u, d[u])), z = d[u] - o;
            const bool b1 = RA[u] >= hs, b2 = RB[u] >= hs;
            const bool u1 = b1 && z != 0, u2 = b2 && hs > z;  // the root's left child is whole (n >= hs)
            lA[u] = u1 ? 1u : lA[u];
            qA[u] = u1 ? z : qA[u];
            lB[u] = u2 ? 1u : lB[u];
            qB[u] = u2 ? z : qB[u];
            cA[u] = b1 ? 0u : o;
            cB[u] = b2 ? 0u : o;
            oA[u] = b1 ? o : z;
            oB[u] = b2 ? o : z;
        }
        uint32_t h = wt_v(hs >> 1), msk = wt_v(~(hs - 1)), l1 = wt_v(2u);
        const uint2 *__restrict__ lvl = lv + nw;
        for (uint32_t l = 1; l < lb; ++l) {
#pragma unroll
            for (int u = 0; u < NS; ++u) {
                const uint32_t s1 = RA[u] & msk, p1 = s1 + oA[u], s2 = RB[u] & msk, p2 = s2 + oB[u];
                const uint2 w1 = lvl[p1 >> five], w2 = lvl[p2 >> five];
                const uint32_t o1 = w1.y + __popc(__builtin_amdgcn_ubfe(w1.x, 0u, p1)) - (s1 >> one);
                const uint32_t o2 = w2.y + __popc(__builtin_amdgcn_ubfe(w2.x, 0u, p2)) - (s2 >> one);
                const uint32_t z1 = oA[u] - o1, z2 = oB[u] - o2;
                const bool b1 = RA[u] & h, b2 = RB[u] & h;
                const bool u1 = b1 && z1 != 0;
                const bool u2 = b2 && min(nv - s2, h) > z2;  // zeros of the node past the prefix: suffix elements < R_B
                lA[u] = u1 ? l1 : lA[u];  // (the node start there is R & msk of that level: rebuilt from lA below)
                qA[u] = u1 ? z1 : qA[u];
                lB[u] = u2 ? l1 : lB[u];
                qB[u] = u2 ? z2 : qB[u];
                cA[u] += b1 ? 0u : o1;
                cB[u] += b2 ? 0u : o2;
                oA[u] = b1 ? o1 : z1;
                oB[u] = b2 ? o2 : z2;
            }
            h >>= 1;
            msk = (uint32_t)((int32_t)msk >> 1);
            l1 += 1;
            lvl += nw;
        }
    }
    // R's rank block: its node's first o entries are the prefix part's elements in it (mk: their ranks' bits), so
    // the ranks >= R among them finish the counts, and those below R hold the part's predecessor when any are there
    MT belA[NS], belB[NS];
    bool hitA[NS], hitB[NS];
    uint32_t l0 = WT_NONE;
#pragma unroll
    for (int u = 0; u < NS; ++u) {
        const uint32_t bA = RA[u] & ~BM, bB = RB[u] & ~BM, rA = RA[u] & BM, rB = RB[u] & BM;
        const MT mA = MK::load(mk, bA + (bA >> BB) + oA[u]), mB = MK::load(mk, bB + (bB >> BB) + oB[u]);
        cA[u] += MK::count_ge(mA, rA);
        cB[u] += MK::count_ge(mB, rB);
        W[u] += cA[u] + (n - RB[u]) - cB[u];
        belA[u] = MK::below(mA, rA);
        belB[u] = MK::below(MK::inv(mB), rB);
        // predecessors: in R's block when a part has an element below R there; else from the deepest branch-off
        // level down to a block (second descent: the prefix part takes the largest rank among the first qA entries of
        // node sA, the suffix part the largest among entries qB.. of node sB); a part with nothing below its bound
        // wraps, and its maximum is its largest rank overall: the same descent from the root (node 0, the part's
        // positions [0, d) or [d, n)). Levels no lane of the wave needs are skipped. (A per-d table of the parts'
        // largest ranks answered the wrap case with one read but cost 4 B per event of the row image.)
        hitA[u] = MK::any(belA[u]);
        hitB[u] = MK::any(belB[u]);
        wrapA[u] = d[u] > 0 && !hitA[u] && lA[u] == WT_NONE;
        wrapB[u] = d[u] < n && !hitB[u] && lB[u] == WT_NONE;
        if (wrapA[u]) {
            lA[u] = 0;
            qA[u] = d[u];
        }
        if (wrapB[u]) {
            lB[u] = 0;
            qB[u] = d[u];
        }
        const bool dA = d[u] > 0 && !hitA[u], dB = d[u] < n && !hitB[u];
        if (!dA) lA[u] = lb;
        if (!dB) lB[u] = lb;
        // the branch-off node: the left child recorded at level lA - 1 starts at R & ~(2^(K - lA + 1) - 1)
        sA[u] = RA[u] & ~((2u << (K - lA[u])) - 1u);
        sB[u] = RB[u] & ~((2u << (K - lB[u])) - 1u);
        l0 = min(l0, min(lA[u], lB[u]));
    }
    if (__builtin_amdgcn_ballot_w64(l0 < lb)) {
        for (uint32_t l = 0; l < lb; ++l) {
            if (!__builtin_amdgcn_ballot_w64(l >= l0)) continue;
            const uint32_t hs = 1u << (K - l - 1);
            const uint32_t h = wt_v(hs), h2 = wt_v(2 * hs), lv1 = wt_v(l);
            const uint2 *__restrict__ lvl = lv + l * nw;
#pragma unroll
            for (int u = 0; u < NS; ++u) {
                const uint32_t p1 = sA[u] + qA[u], p2 = sB[u] + qB[u];
                const uint2 w1 = lvl[p1 >> five], w2 = lvl[p2 >> five];
                const uint32_t o1 = w1.y + __popc(__builtin_amdgcn_ubfe(w1.x, 0u, p1)) - (sA[u] >> one);
                const uint32_t o2 = w2.y + __popc(__builtin_amdgcn_ubfe(w2.x, 0u, p2)) - (sB[u] >> one);
                const bool a1 = lv1 >= lA[u], a2 = lv1 >= lB[u];
                const bool g1 = a1 && o1 != 0;
                const bool g2 = a2 && min(nv - sB[u], h2) > h + o2;  // ones of the node past the prefix
                sA[u] += g1 ? h : 0u;
                qA[u] = g1 ? o1 : qA[u];
                sB[u] += g2 ? h : 0u;
                qB[u] = a2 ? (g2 ? o2 : qB[u] - o2) : qB[u];
            }
        }
    }
    // the descended lanes end in a block: the prefix part's elements are its first qA entries, the suffix part's the
    // entries from qB on (of the block's min(n - sB, 32))
#pragma unroll
    for (int u = 0; u < NS; ++u) {
        const MT vA = MK::load(mk, sA[u] + (sA[u] >> BB) + qA[u]);
        const MT vB = MK::low(MK::inv(MK::load(mk, sB[u] + (sB[u] >> BB) + qB[u])), min(nv - sB[u], BW));
        const uint32_t bA = RA[u] & ~BM, bB = RB[u] & ~BM;
        pA[u] = hitA[u] ? bA + MK::top(belA[u]) : sA[u] + MK::top(vA);
        pB[u] = hitB[u] ? bB + MK::top(belB[u]) : sB[u] + MK::top(vB);
    }
    }
    // (5) the parts' maxima {t, ~e}: each part's base plus the Cm at its rank, less m when the part wraps
#pragma unroll
    for (int u = 0; u < NS; ++u) {
        if (d[u] > 0) {
            const uint32_t t = Hm[u] + cm[pA[u]] - (wrapA[u] ? m : 0u);
            const uint64_t k = ((uint64_t)t << 32) | (0xffffffffu - ev[pA[u]]);
            key[u] = k > key[u] ? k : key[u];
        }
        if (d[u] < n) {
            const uint32_t t = Hm2[u] + cm[pB[u]] - (wrapB[u] ? m : 0u);
            const uint64_t k = ((uint64_t)t << 32) | (0xffffffffu - ev[pB[u]]);
            key[u] = k > key[u] ? k : key[u];
        }
        sum[u] += (uint64_t)d[u] * Hm[u] + (uint64_t)(n - d[u]) * Hm2[u];
    }
}

#ifdef WT_TRACE
// timing-only builds (-DWT_TRACE, G = 1): wall_clock64 per (row, wave) at the kernel start [9], after staging [0] and
// at the end of each of up to 8 chunks [1..8]; read with nmz_debug_wt_trace (tools/k1_trace.py --wt)
__device__ unsigned long long g_wt_trace[256][16][10];
#define WT_TSTAMP(slot)                                                                                      \
    do {                                                                                                     \
        if ((threadIdx.x & 63) == 0 && blockIdx.x < 256 && (slot) < 10)                                      \
            g_wt_trace[blockIdx.x][threadIdx.x >> 6][(slot)] = wall_clock64();                               \
    } while (0)
#else
#define WT_TSTAMP(slot) \
    do {                \
    } while (0)
#endif

// G workgroups per row L: each stages the row image into LDS and takes a contiguous share of the row's chunks of
// 64 NS seeds (NS per lane), which its waves take one at a time from an LDS counter; with rec, every chunk leaves its
// record for the selection (replayable_wt_topk_dev.h).
// The row image (~84 KB at configs[1]) allows one workgroup (16 waves, 4 per SIMD) per CU.
template <bool BIG, int NS, int BB, bool PL = false>
__global__ __launch_bounds__(1024) void k_replayable_sweep_wt(
    const uint32_t *__restrict__ bucket_off, const uint64_t *__restrict__ sorted_h0,
    const uint32_t *__restrict__ sorted_idx, const uint4 *__restrict__ table, uint32_t E,
    const uint4 *__restrict__ blob, uint32_t rb16, const unsigned long long *__restrict__ rowsum,
    const WtClass *__restrict__ classes, uint32_t n_classes, uint32_t m, uint64_t mu, uint32_t m_k64, uint32_t msh,
    uint32_t G, nmz_sched_stats *__restrict__ stats, unsigned long long *__restrict__ span,
    WtChunkRec *__restrict__ rec) {
    constexpr uint32_t CS = 64 * NS;  // seeds per chunk
    extern __shared__ uint4 wt_lds[];
    const uint32_t L = blockIdx.x / G, g = blockIdx.x % G;
    const uint32_t s0 = bucket_off[L], s1 = bucket_off[L + 1];
    const uint32_t nch = (s1 - s0 + CS - 1) / CS;
    const uint32_t c0 = g * nch / G, c1 = (g + 1) * nch / G;
    uint32_t *ctr = reinterpret_cast<uint32_t *>(wt_lds + rb16);  // [0] the chunk counter, [4..7] chunk_base parts
    if (c0 == c1) return;  // no chunks (and no records) of this group
    if (span && threadIdx.x == 0) atomicMax(span, ~(unsigned long long)wall_clock64());
    WT_TSTAMP(9);
    // chunk_base[L], the chunks of the rows before L: the first 256 threads add up a row's chunks each (loaded here,
    // under the staging), their waves leave partial sums in LDS before the staging's barrier
    uint32_t cb = 0;
    if (rec)
        for (uint32_t t = threadIdx.x; t < L; t += blockDim.x) cb += (bucket_off[t + 1] - bucket_off[t] + CS - 1) / CS;
    {
        const uint4 *__restrict__ src = blob + (uint64_t)L * rb16;
        // every load of a pass in flight at once (indices clamped to the image, stores unconditional)
        constexpr uint32_t B = 8;
        const uint32_t nt = blockDim.x;
        for (uint32_t i0 = 0; i0 < rb16; i0 += B * nt) {
            uint4 v[B];
#pragma unroll
            for (uint32_t k = 0; k < B; ++k) v[k] = src[min(i0 + k * nt + threadIdx.x, rb16 - 1)];
#pragma unroll
            for (uint32_t k = 0; k < B; ++k) wt_lds[min(i0 + k * nt + threadIdx.x, rb16 - 1)] = v[k];
        }
        if (threadIdx.x == 0) *ctr = c0;
        if (rec && threadIdx.x < 256) {
            for (int o = 32; o; o >>= 1) cb += __shfl_xor(cb, o, 64);
            if ((threadIdx.x & 63) == 0) ctr[4 + (threadIdx.x >> 6)] = cb;
            if (threadIdx.x < 4 && threadIdx.x >= nt / 64) ctr[4 + threadIdx.x] = 0;  // fewer than four waves
        }
    }
    __syncthreads();
    const uint32_t cbase = rec ? __builtin_amdgcn_readfirstlane(ctr[4] + ctr[5] + ctr[6] + ctr[7]) : 0u;
    WT_TSTAMP(0);
#ifdef WT_TRACE
    uint32_t n_done = 0;
#endif
    const char *img = reinterpret_cast<const char *>(wt_lds);
    const uint4 *__restrict__ row = table + (uint64_t)L * E;
    const uint64_t rsum = rowsum[L];
    const uint32_t lane = threadIdx.x & 63;
    WtVConst vc;
#pragma unroll
    for (int r = 0; r < 5; ++r) vc.st4[r] = wt_v(4u << r);
    // chunks from the LDS counter; the next chunk's seeds and indices are loaded while this one runs
    uint32_t ch = 0;
    if (lane == 0) ch = atomicAdd(ctr, 1u);
    ch = __builtin_amdgcn_readfirstlane(ch);
    uint64_t h0n[NS];
    uint32_t idxn[NS];
#pragma unroll
    for (int u = 0; u < NS; ++u) {
        const uint32_t jn = min(s0 + ch * CS + u * 64 + lane, s1 - 1);  // past the share: a valid seed, unused
        h0n[u] = sorted_h0[jn];
        idxn[u] = sorted_idx[jn];
    }
    while (ch < c1) {
        const uint32_t j0 = s0 + ch * CS + lane;
        uint64_t h0[NS];
        uint32_t idx[NS];
#pragma unroll
        for (int u = 0; u < NS; ++u) {
            h0[u] = h0n[u];
            idx[u] = idxn[u];
        }
        uint32_t chn = 0;
        if (lane == 0) chn = atomicAdd(ctr, 1u);
        chn = __builtin_amdgcn_readfirstlane(chn);
#pragma unroll
        for (int u = 0; u < NS; ++u) {
            const uint32_t jn = min(s0 + chn * CS + u * 64 + lane, s1 - 1);
            h0n[u] = sorted_h0[jn];
            idxn[u] = sorted_idx[jn];
        }
        uint64_t sum[NS], key[NS];
        uint32_t W[NS];
#pragma unroll
        for (int u = 0; u < NS; ++u) sum[u] = key[u] = W[u] = 0;
        for (uint32_t c = 0; c < n_classes; ++c)
            wt_seed_class<BIG, NS, BB, PL>(vc, classes[c], img, row, h0, m, mu, m_k64, msh, sum, W, key);
        uint64_t km = 0;  // the chunk's largest sum, in the top-k's order (int64, as an order-preserving u64 key)
#pragma unroll
        for (int u = 0; u < NS; ++u) {
            const uint32_t j = j0 + u * 64;
            const uint64_t total = sum[u] + rsum - (uint64_t)W[u] * m;
            if (j < s1) {
                const uint64_t kk = total ^ (1ull << 63);
                km = kk > km ? kk : km;
                nmz_sched_stats st;
                st.sum_delay_ns = total;
                st.max_delay_ns = (int64_t)(key[u] >> 32);
                st.argmax_event = ~(uint32_t)key[u];
                st.n_fault = 0;
                st.first_fault = NMZ_NONE;
                st.flags = 0;
                stats[idx[u]] = st;
            }
        }
        if (rec) {  // the chunk's record, one 16-byte store
            for (int o = 32; o; o >>= 1) {
                const uint64_t v = __shfl_xor(km, o, 64);
                km = v > km ? v : km;
            }
            const uint32_t p = s0 + ch * CS;
            if (lane == 0)
                reinterpret_cast<uint4 *>(rec)[cbase + ch] =
                    make_uint4((uint32_t)km, (uint32_t)(km >> 32), p, min(CS, s1 - p));
        }
#ifdef WT_TRACE
        if (++n_done <= 8) WT_TSTAMP(n_done);
#endif
        ch = chn;
    }
    if (span) {
        __syncthreads();
        if (threadIdx.x == 0) atomicMax(span + 1, (unsigned long long)wall_clock64());
    }
}

}  // namespace nmz

#include "replayable_wt_topk_dev.h"  // k_wt_topk_chunks, the selection over the chunk records

namespace nmz {

// ---------------------------------------------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------------------------------------------
// workgroups per row and threads per workgroup (A/B knobs NMZ_WT_G = 1|2|4|8, NMZ_WT_THREADS = 64..1024)
static uint32_t wt_groups() {
    static const uint32_t g = [] {
        // one workgroup per row leaves half of each CU's wave slots and LDS to the step's other kernels (the seed
        // prefix, bucketing and top-k of the neighbouring pipelined steps): configs[1] step 0.116 -> 0.113 ms with
        // the fused top-k (profiles/r03y_wt_groups_ab.json); alone, 2 per row are 2 % faster
        const char *e = ab_env("NMZ_WT_G");
        const int v = e ? atoi(e) : 1;
        return (uint32_t)((v == 1 || v == 2 || v == 4 || v == 8) ? v : 1);
    }();
    return g;
}
static uint32_t wt_threads() {
    static const uint32_t t = [] {
        const char *e = ab_env("NMZ_WT_THREADS");
        const int v = e ? atoi(e) : 1024;
        return (uint32_t)((v >= 64 && v <= 1024 && v % 64 == 0) ? v : 1024);
    }();
    return t;
}

// the sweep's forms: every launch and the LDS attribute take the kernel from here (planes: 64-rank blocks only).
// One seed per lane: two (NS = 2, 106 VGPRs) measured slower, K1 span 0.074 vs 0.059 ms
// (profiles/r04/k1_ns2_rejected/)
using WtSweepKernel = decltype(&k_replayable_sweep_wt<false, WT_NS, 5>);
template <bool BIG>
static WtSweepKernel wt_sweep_kernel_of(uint32_t bb, bool planes) {
    return bb == 7   ? k_replayable_sweep_wt<BIG, WT_NS, 7>
           : bb == 6 ? (planes ? k_replayable_sweep_wt<BIG, WT_NS, 6, true> : k_replayable_sweep_wt<BIG, WT_NS, 6>)
                     : k_replayable_sweep_wt<BIG, WT_NS, 5>;
}
static WtSweepKernel wt_sweep_kernel(bool big, uint32_t bb, bool planes) {
    return big ? wt_sweep_kernel_of<true>(bb, planes) : wt_sweep_kernel_of<false>(bb, planes);
}
bool wt_sweep_lds_attr() {
    for (bool big : {false, true})
        for (uint32_t bb = 5; bb <= 7; ++bb)
            for (bool planes : {false, true})
                if (hipFuncSetAttribute(reinterpret_cast<const void *>(wt_sweep_kernel(big, bb, planes)),
                                        hipFuncAttributeMaxDynamicSharedMemorySize, (int)WT_LDS_MAX) != hipSuccess)
                    return false;
    return true;
}

// topk_scratch (wt_topk_scratch_bytes(S)) or nullptr: the sweep also leaves its chunk records there for wt_topk
int wt_sweep(const WtState &w, nmz_ctx *ctx, hipStream_t st, const Buckets &b, const uint4 *d_table, uint32_t E,
             const ModParams &mod, nmz_sched_stats *d_stats, uint64_t S, void *topk_scratch) {
    WtChunkRec *rec = wt_topk_carve(topk_scratch, S).rec;
    const uint32_t G = wt_groups(), nt = wt_threads();
    KernelTimer kt(ctx, st, "replayable_sweep");
    unsigned long long *span = kt.span();
    const size_t lds = w.rb16 * 16u + 32u;
    hipLaunchKernelGGL(wt_sweep_kernel(mod.m32 >= 0x80000000u, w.bb, w.planes), dim3(256 * G), dim3(nt), lds, st,
                       b.offset, b.sorted_h0, b.sorted_idx, d_table, E, w.d_blob, w.rb16, w.d_rowsum,
                       static_cast<const WtClass *>(w.d_classes), w.n_classes, mod.m32, mod.mu, mod.m_k64, w.msh, G,
                       d_stats, span, rec);
    NMZ_HIP(hipGetLastError());
    return NMZ_OK;
}

size_t wt_topk_scratch_bytes(uint64_t S) { return wt_topk_carve(nullptr, S).bytes; }

// the selection after a sweep that ran with this scratch (its chunk records) over the seeds bucketed as bucket_off
// and sorted_idx say, with the sweep's stats
int wt_topk(hipStream_t st, void *scratch, const uint32_t *bucket_off, const uint32_t *sorted_idx,
            const nmz_sched_stats *d_stats, uint64_t S, uint64_t seed0, uint32_t k, nmz_topk_entry *d_out) {
    NMZ_CHECK(k >= 1 && k <= 64, "internal: wt_topk takes 1 <= k <= 64");
    const WtTopkScratch sc = wt_topk_carve(scratch, S);
    hipLaunchKernelGGL(k_wt_topk_chunks<64 * WT_NS>, dim3(1), dim3(WT_SEL_THREADS), 0, st, bucket_off,
                       static_cast<const WtChunkRec *>(sc.rec), sorted_idx, d_stats, S, seed0, k,
                       (uint32_t)wt_max_chunks(S), sc.tk, d_out);
    NMZ_HIP(hipGetLastError());
    return NMZ_OK;
}

}  // namespace nmz

#ifdef WT_TRACE
extern "C" int nmz_debug_wt_trace(unsigned long long *out) {
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(nmz::g_wt_trace), sizeof(nmz::g_wt_trace)) == hipSuccess ? 0 : -1;
}
#endif
