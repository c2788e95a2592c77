// K1 -- the per-decision sweeps: every (seed, event) decision computed one by one. k_replayable_sweep_fast (with
// k_replayable_merge) for 0 < m < 2^30, k_replayable_sweep_general for any other m > 0. The statistics kernels
// (replayable_wt.hip, replayable_oq.hip) run instead wherever they apply; these are the reference they are
// measured against and the path for plans that neither fits. replayable.hip explains the algebra (steps 3-5).
#include <algorithm>

#include "nmz_common.h"
#include "nmz_internal.h"
#include "replayable_plan.h"

namespace nmz {

// seeds per lane. 2 is the fastest measured (4 and 8 were tried); the argmax key is kept as f64 bits folded with
// v_max_f64: 0.83 ms per launch on configs[1] against 0.96 ms for a u64 compare chain (and 0.98 ms for a
// strict-greater update on t with a tie flag -- 11 full-rate VOP2 per decision, no v_subb / v_max)
constexpr int REPLAY_U = 2;
static_assert(64 * REPLAY_U == REPLAY_SEEDS_PER_UNIT_MIN, "the seed scratch's unit list is sized for 64 * REPLAY_U");
// persistent workgroups (4 waves each) per CU: 8 = 8 waves/SIMD (K1 0.836-0.843 ms; 7: 0.833-0.856, 6: 0.889,
// 5: 0.905-0.943, profiles/r02t_k1_wg_ab.log)
constexpr uint32_t REPLAY_WG_PER_CU = 8;
constexpr uint32_t REPLAY_EC = 2048;  // events per work item (2048 vs 1024: same sweep time, half the merge reads)

// ---------------------------------------------------------------------------
// the sweep (MOD_FAST): persistent waves take work items of up to 64*U seeds
// (U per lane) that share the FNV low byte L, times a chunk of events.
// ---------------------------------------------------------------------------
__device__ __forceinline__ uint32_t vgpr(uint32_t x) {
    // keep a launch constant in a VGPR: VGPR-only VOP2 issues at full rate,
    // the SGPR / literal operand forms at half rate on gfx950
    uint32_t v;
    asm volatile("v_mov_b32 %0, %1" : "=v"(v) : "s"(x));
    return v;
}

__device__ __forceinline__ void vsub(uint32_t &d, uint32_t x) {
    asm("v_sub_u32 %0, %0, %1" : "+v"(d) : "v"(x));
}

// One decision, VOP2 carry/borrow chains only (the forms gfx950 issues at
// ~2.25 cycles; v_cmp_*, v_min/max_u32 and v_addc/v_subb take ~4.1 --
// tools/ubench/valu_patterns.hip, decide_block.hip):
//   vcc = T_t < d                 v_sub_co     (before the seed's carry switch)
//   s   = (vcc ? Hm : Hm2) + Cm   v_cndmask, v_add
//   t   = s < m ? s : s - m       v_sub_co (borrow), v_cndmask
//   part += t                     v_add
//   key = max(key, t:~e)          v_max_f64
// The argmax key is kept as the bit pattern of an f64:
// (t << 32 | ~e) with t < 2^30 is a non-negative finite double (bit 63 = 0,
// exponent < 0x7ff; f64 denormals are preserved, the kernel default), whose
// order equals the u64 order, so a 4-instruction u64 compare/select
// becomes one v_max_f64.
__device__ __forceinline__ void decide_f64(uint32_t Tt, uint32_t d, uint32_t Hm, uint32_t Hm2, uint2 q, uint32_t mv,
                                           double &kmax, uint32_t &part) {
    // q = {~e, C mod m}, this seed's own copy from LDS; t replaces C mod m in
    // place, so {~e, t} is already the key's register pair (no v_mov)
    uint32_t t0, tmp, cv;
    uint32_t x = q.y;
    asm("v_sub_co_u32 %[t0], vcc, %[Tt], %[d]\n\t"
        "v_cndmask_b32 %[tmp], %[Hm2], %[Hm], vcc\n\t"
        "v_add_u32 %[x], %[x], %[tmp]\n\t"
        "v_sub_co_u32 %[cv], vcc, %[x], %[mv]\n\t"
        "v_cndmask_b32 %[x], %[cv], %[x], vcc\n\t"
        "v_add_u32 %[part], %[part], %[x]"
        : [t0] "=&v"(t0), [tmp] "=&v"(tmp), [cv] "=&v"(cv), [x] "+v"(x), [part] "+v"(part)
        : [Tt] "v"(Tt), [d] "v"(d), [Hm] "v"(Hm), [Hm2] "v"(Hm2), [mv] "v"(mv)
        : "vcc");
    const double key = __builtin_bit_cast(double, ((uint64_t)x << 32) | q.x);
    asm("v_max_f64 %0, %0, %1" : "+v"(kmax) : "v"(key));
}

// Four decisions of one seed (events T0..T3 of a group) in one asm block: the hazard recognizer
// treats each inline asm conservatively (an s_nop at block boundaries), so one block per four
// decisions instead of one per decision. t overwrites each event's C mod m in place; the four
// keys {~e, t} are folded by key_max4 afterwards, 4+ instructions after their last write
// (0.83 -> 0.80 ms per launch).
__device__ __forceinline__ void decide4(uint32_t T0, uint32_t T1, uint32_t T2, uint32_t T3, uint32_t d, uint32_t Hm,
                                        uint32_t Hm2, uint32_t mv, uint32_t &x0, uint32_t &x1, uint32_t &x2,
                                        uint32_t &x3, uint32_t &part) {
    uint32_t t0, tmp, cv;
#define NMZ_DEC(T, X)                                  \
    "v_sub_co_u32 %[t0], vcc, " T ", %[d]\n\t"         \
    "v_cndmask_b32 %[tmp], %[Hm2], %[Hm], vcc\n\t"     \
    "v_add_u32 " X ", " X ", %[tmp]\n\t"               \
    "v_sub_co_u32 %[cv], vcc, " X ", %[mv]\n\t"        \
    "v_cndmask_b32 " X ", %[cv], " X ", vcc\n\t"       \
    "v_add_u32 %[part], %[part], " X "\n\t"
    asm(NMZ_DEC("%[T0]", "%[x0]") NMZ_DEC("%[T1]", "%[x1]") NMZ_DEC("%[T2]", "%[x2]") NMZ_DEC("%[T3]", "%[x3]")
        : [t0] "=&v"(t0), [tmp] "=&v"(tmp), [cv] "=&v"(cv), [x0] "+v"(x0), [x1] "+v"(x1), [x2] "+v"(x2),
          [x3] "+v"(x3), [part] "+v"(part)
        : [T0] "v"(T0), [T1] "v"(T1), [T2] "v"(T2), [T3] "v"(T3), [d] "v"(d), [Hm] "v"(Hm), [Hm2] "v"(Hm2),
          [mv] "v"(mv)
        : "vcc");
#undef NMZ_DEC
}

__device__ __forceinline__ void key_max4(double &kmax, double a, double b, double c, double d) {
    asm("v_max_f64 %0, %0, %1\n\t"
        "v_max_f64 %0, %0, %2\n\t"
        "v_max_f64 %0, %0, %3\n\t"
        "v_max_f64 %0, %0, %4"
        : "+v"(kmax)
        : "v"(a), "v"(b), "v"(c), "v"(d));
}

// number of entries in the C-sorted range row[lo, lo+n) with C <= x
__device__ __forceinline__ uint32_t count_le(const uint4 *__restrict__ row, uint32_t lo, uint32_t n, uint64_t x) {
    uint32_t k = 0;
    for (uint32_t s = n ? 1u << (31 - __builtin_clz(n)) : 0u; s; s >>= 1) {
        if (k + s <= n) {
            const uint2 c = *reinterpret_cast<const uint2 *>(row + lo + k + s - 1);
            if ((((uint64_t)c.y << 32) | c.x) <= x) k += s;
        }
    }
    return k;
}

// seed r's {~e, C mod m} pair from a 16-B staged read holding seeds 2k, 2k+1
__device__ __forceinline__ uint2 half_of(uint4 v, int hi) { return hi ? make_uint2(v.z, v.w) : make_uint2(v.x, v.y); }

constexpr uint32_t POS_BIAS = 0x40000000u;  // keeps d = BIAS + k - i positive

// Work item = (seed group of <= 64*U seeds sharing the low byte L, chunk of
// `ec` events in the table order). Items are handed out dynamically (one
// global atomic per item) to a persistent grid, so the last round is never a
// half-empty second pass; each item writes its partial (sum, key) per seed
// and k_replayable_merge combines the chunks.
template <int U>
__global__ __launch_bounds__(256) void k_replayable_sweep_fast(
    const uint4 *__restrict__ units, const uint32_t *__restrict__ n_units,
    const uint64_t *__restrict__ sorted_h0, const uint4 *__restrict__ table, uint32_t E,
    const ClassInfo *__restrict__ classes, uint32_t n_classes, uint64_t m, uint64_t m_mu, uint32_t m_k64, uint32_t ec,
    uint32_t n_chunks, uint32_t fold_mask, uint32_t *__restrict__ item_counter, uint4 *__restrict__ partial,
    uint64_t part_stride) {
    // per-wave double-buffered staging of 64 table entries in LDS: one
    // coalesced 16-B load per lane fetches the next chunk while the current
    // one is consumed through broadcast LDS reads. An event's slot holds
    // {~e, C mod m} x U: every seed r reads its own pair, and the decision
    // overwrites C mod m with t, leaving the f64 key pair {~e, t} in place.
    static_assert(U % 2 == 0, "staged reads take seeds in pairs");
    constexpr int STR = 2 * U;
    __shared__ __attribute__((aligned(16))) uint32_t stage[4][2][64 * STR];
    const uint32_t wv = threadIdx.x >> 6;
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t m32 = (uint32_t)m;
    const uint32_t mv = vgpr(m32);
    const uint32_t T0 = vgpr(POS_BIAS), T1 = vgpr(POS_BIAS + 1), T2 = vgpr(POS_BIAS + 2), T3 = vgpr(POS_BIAS + 3);
    const uint32_t V4 = vgpr(4u), V1 = vgpr(1u);
    const uint32_t n_items = *n_units * n_chunks;
    uint32_t slot = 0;

    for (;;) {
        uint32_t item = 0;
        if (lane == 0) item = atomicAdd(item_counter, 1u);
        item = __builtin_amdgcn_readfirstlane(__shfl(item, 0, 64));
        if (item >= n_items) break;
        const uint32_t unit = item / n_chunks, chunk = item - unit * n_chunks;
        const uint4 u = units[unit];
        const uint32_t L = __builtin_amdgcn_readfirstlane(u.x);
        const uint32_t start = __builtin_amdgcn_readfirstlane(u.y);
        const uint32_t cnt = __builtin_amdgcn_readfirstlane(u.z);
        const uint32_t e0 = chunk * ec, e1 = min(E, e0 + ec);

        uint64_t h0[U];
        uint32_t sum_lo[U], sum_hi[U];
        double kf[U];  // key = max of (t << 32 | ~e) as f64 bits; 0 = none
#pragma unroll
        for (int r = 0; r < U; ++r) {
            const uint32_t j = lane + 64 * r;
            h0[r] = (j < cnt) ? sorted_h0[start + j] : 0;
            sum_lo[r] = 0;
            sum_hi[r] = 0;
            kf[r] = 0.0;
        }
        const uint4 *__restrict__ row = table + (uint64_t)L * E;

        // class containing e0 (few classes: scalar scan)
        uint32_t cc = 0;
        ClassInfo ci = classes[0];
        while (ci.start + ci.count <= e0) ci = classes[++cc];
        uint32_t pos = e0;  // next event (table order) to stage
        uint32_t hi_c = min(e1, ci.start + ci.count);
        uint4 pre = (pos + lane < hi_c) ? row[pos + lane] : make_uint4(0, 0, 0, 0);
        uint32_t Hm[U], Hm2[U], d[U];
        bool fresh = true;
        while (pos < e1) {
            if (fresh) {
#pragma unroll
                for (int r = 0; r < U; ++r) {
                    const uint64_t H = h0[r] * ci.pn;
                    Hm[r] = mod_barrett_small(H, m32, m_mu);
                    const uint32_t t2 = Hm[r] + m_k64;
                    Hm2[r] = min(t2, t2 - m32);
                    // carry(H + C) <=> C > ~H <=> position >= pos + count(C <= ~H)
                    d[r] = POS_BIAS + count_le(row, pos, hi_c - pos, ~H);
                }
                fresh = false;
            }
            const uint32_t n = min(64u, hi_c - pos);
            {
                uint32_t *sw = &stage[wv][slot][lane * STR];
#pragma unroll
                for (int r = 0; r < U; ++r) {
                    sw[2 * r] = pre.w;
                    sw[2 * r + 1] = pre.z;
                }
            }
            // prefetch the next staged chunk (possibly in the next class)
            uint32_t npos = pos + n, nhi = hi_c;
            ClassInfo nci = ci;
            bool nfresh = false;
            if (npos == hi_c && npos < e1) {
                nci = classes[cc + 1];
                nhi = min(e1, nci.start + nci.count);
                nfresh = true;
            }
            // unconditional and clamped to the row: a guarded load became a divergent block whose result
            // the compiler waited for (s_waitcnt vmcnt(0)) right after issuing it. Slots past the chunk's
            // n events are never read, so the clamped lanes' values do not matter.
            pre = row[min(npos + lane, E - 1)];
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            const uint32_t *__restrict__ sq = stage[wv][slot];
            const uint32_t n4 = n & ~3u;
            // part[r] holds up to 4 << fold_shift delays (< 2^32 since t < m) between folds
            uint32_t part[U];
#pragma unroll
            for (int r = 0; r < U; ++r) part[r] = 0;
            for (uint32_t i = 0, g = 1; i < n4; i += 4, ++g) {
                double kk[U][4];
                // the 4 events' slots as 16-B reads (ds_read_b128: one LDS pass per 4 lane groups,
                // half the LDS cycles of the ds_read2_b64 pairs that 8-B reads compile to)
                uint4 qv[U / 2][4];
#pragma unroll
                for (int rr = 0; rr < U / 2; ++rr)
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        qv[rr][j] = *reinterpret_cast<const uint4 *>(sq + (i + j) * STR + 4 * rr);
#pragma unroll
                for (int r = 0; r < U; ++r) {
                    const uint2 q0 = half_of(qv[r / 2][0], r & 1), q1 = half_of(qv[r / 2][1], r & 1);
                    const uint2 q2 = half_of(qv[r / 2][2], r & 1), q3 = half_of(qv[r / 2][3], r & 1);
                    uint32_t x0 = q0.y, x1 = q1.y, x2 = q2.y, x3 = q3.y;
                    decide4(T0, T1, T2, T3, d[r], Hm[r], Hm2[r], mv, x0, x1, x2, x3, part[r]);
                    kk[r][0] = __builtin_bit_cast(double, ((uint64_t)x0 << 32) | q0.x);
                    kk[r][1] = __builtin_bit_cast(double, ((uint64_t)x1 << 32) | q1.x);
                    kk[r][2] = __builtin_bit_cast(double, ((uint64_t)x2 << 32) | q2.x);
                    kk[r][3] = __builtin_bit_cast(double, ((uint64_t)x3 << 32) | q3.x);
                    vsub(d[r], V4);
                }
#pragma unroll
                for (int r = 0; r < U; ++r) key_max4(kf[r], kk[r][0], kk[r][1], kk[r][2], kk[r][3]);
                if ((g & fold_mask) == 0) {
#pragma unroll
                    for (int r = 0; r < U; ++r) {
                        const uint32_t lo = sum_lo[r] + part[r];
                        sum_hi[r] += (lo < part[r]);
                        sum_lo[r] = lo;
                        part[r] = 0;
                    }
                }
            }
            for (uint32_t i = n4; i < n; ++i) {  // class / item tail (< 4 events)
#pragma unroll
                for (int r = 0; r < U; ++r) {
                    const uint2 q1 = *reinterpret_cast<const uint2 *>(sq + i * STR + 2 * r);
                    decide_f64(T0, d[r], Hm[r], Hm2[r], q1, mv, kf[r], part[r]);
                    vsub(d[r], V1);
                }
            }
            // here part holds <= fold_mask groups since the last fold plus the tail
            // (< 4 events): fewer than 4 * (fold_mask + 1) delays, so no overflow
#pragma unroll
            for (int r = 0; r < U; ++r) {
                const uint32_t lo = sum_lo[r] + part[r];
                sum_hi[r] += (lo < part[r]);
                sum_lo[r] = lo;
            }
            slot ^= 1;
            pos = npos;
            if (nfresh) {
                ci = nci;
                ++cc;
                hi_c = nhi;
                fresh = true;
            }
        }
        uint4 *__restrict__ out = partial + (uint64_t)chunk * part_stride + (uint64_t)unit * (64 * U);
#pragma unroll
        for (int r = 0; r < U; ++r) {
            const uint64_t kb = __builtin_bit_cast(uint64_t, kf[r]);
            out[lane + 64 * r] = make_uint4(sum_lo[r], sum_hi[r], (uint32_t)kb, (uint32_t)(kb >> 32));
        }
    }
}

// combine the per-chunk partials of slot g (unit g / 64U, lane-seed g % 64U); false for empty slots
template <int U>
__device__ __forceinline__ bool merge_slot(uint64_t g, const uint4 *__restrict__ units, uint32_t n_units,
                                          const uint32_t *__restrict__ sorted_idx, const uint4 *__restrict__ partial,
                                          uint64_t part_stride, uint32_t n_chunks, nmz_sched_stats &st,
                                          uint32_t &idx) {
    const uint64_t unit = g / (64 * U);
    const uint32_t j = (uint32_t)(g - unit * (64 * U));
    if (unit >= n_units) return false;
    const uint4 u = units[unit];
    if (j >= u.z) return false;
    uint64_t sum = 0, key = 0;
    for (uint32_t c = 0; c < n_chunks; ++c) {
        const uint4 p = partial[(uint64_t)c * part_stride + g];
        sum += ((uint64_t)p.y << 32) | p.x;
        const uint64_t k = ((uint64_t)p.w << 32) | p.z;
        key = k > key ? k : key;
    }
    st.sum_delay_ns = sum;
    st.max_delay_ns = (int64_t)(key >> 32);
    st.argmax_event = ~(uint32_t)key;
    st.n_fault = 0;
    st.first_fault = NMZ_NONE;
    st.flags = 0;
    idx = sorted_idx[u.y + j];
    return true;
}

// combine the per-chunk partials of every seed and scatter to the original index
template <int U>
__global__ __launch_bounds__(256) void k_replayable_merge(const uint4 *__restrict__ units,
                                                          const uint32_t *__restrict__ n_units,
                                                          const uint32_t *__restrict__ sorted_idx,
                                                          const uint4 *__restrict__ partial, uint64_t part_stride,
                                                          uint32_t n_chunks, nmz_sched_stats *__restrict__ stats) {
    const uint64_t g = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    nmz_sched_stats st;
    uint32_t idx;
    if (merge_slot<U>(g, units, *n_units, sorted_idx, partial, part_stride, n_chunks, st, idx)) stats[idx] = st;
}

// general modulus (m >= 2^30, including uint64(negative duration)): one seed per lane
__global__ __launch_bounds__(256) void k_replayable_sweep_general(
    const uint4 *__restrict__ units, const uint32_t *__restrict__ n_units,
    const uint64_t *__restrict__ sorted_h0, const uint32_t *__restrict__ sorted_idx,
    const uint4 *__restrict__ table, uint32_t E, const ClassInfo *__restrict__ classes,
    uint32_t n_classes, uint64_t m, nmz_sched_stats *__restrict__ stats) {
    const uint32_t wave = __builtin_amdgcn_readfirstlane((blockIdx.x * 256 + threadIdx.x) >> 6);
    const uint32_t lane = threadIdx.x & 63;
    if (wave >= *n_units) return;
    const uint4 u = units[wave];
    const uint32_t L = __builtin_amdgcn_readfirstlane(u.x);
    const uint32_t start = __builtin_amdgcn_readfirstlane(u.y);
    const uint32_t cnt = __builtin_amdgcn_readfirstlane(u.z);
    const uint4 *__restrict__ row = table + (uint64_t)L * E;
    for (uint32_t j = lane; j < cnt; j += 64) {
        const uint64_t h0 = sorted_h0[start + j];
        uint64_t sum = 0;
        int64_t best = INT64_MIN;
        uint32_t arg = NMZ_NONE;
        for (uint32_t c = 0; c < n_classes; ++c) {
            const ClassInfo ci = classes[c];
            const uint64_t H = h0 * ci.pn;
            for (uint32_t i = 0; i < ci.count; ++i) {
                const uint4 qq = row[ci.start + i];
                const uint64_t h = H + (((uint64_t)qq.y << 32) | qq.x);
                const int64_t d = (int64_t)(h % m);
                const uint32_t e = ~qq.w;
                sum += (uint64_t)d;
                if (arg == NMZ_NONE || d > best || (d == best && e < arg)) {
                    best = d;
                    arg = e;
                }
            }
        }
        nmz_sched_stats st;
        st.sum_delay_ns = sum;
        st.max_delay_ns = best;
        st.argmax_event = arg;
        st.n_fault = 0;
        st.first_fault = NMZ_NONE;
        st.flags = 0;
        stats[sorted_idx[start + j]] = st;
    }
}

// the per-chunk partial rows of a plan for S seeds and E events
static int partial_bind(DevBuf &buf, uint64_t S, uint32_t E, uint4 **d_partial) {
    const uint64_t units = S / (64 * (uint64_t)REPLAY_U) + 257;
    const uint64_t chunks = (E + REPLAY_EC - 1) / REPLAY_EC;
    ScratchLayout lay;
    return lay.add(d_partial, units * 64 * REPLAY_U * chunks).bind(buf);
}

int pd_sweep(nmz_replayable_plan *p, hipStream_t st, SeedScratch &sc, uint64_t S, nmz_sched_stats *d_stats) {
    const uint32_t E = p->n_events;
    constexpr uint32_t per_unit = 64u * REPLAY_U;
    NMZ_TRY(bucket_seeds_counted(st, sc.h0, S, p->mod.kind == MOD_FAST ? per_unit : 64, sc.b, sc.counter));
    if (p->mod.kind == MOD_FAST) {
        const uint64_t max_units = S / per_unit + 256;
        const uint32_t n_chunks = (E + REPLAY_EC - 1) / REPLAY_EC;
        uint4 *d_partial;
        NMZ_TRY(partial_bind(p->partial, p->max_seeds, E, &d_partial));
        const uint64_t stride = (p->max_seeds / per_unit + 257) * (uint64_t)per_unit;
        // fold the u32 partial sums every 2^f groups of 4 events, (4 << f)(m - 1) + 3(m - 1) < 2^32
        uint32_t fold_mask = 0;
        while (fold_mask < 15 && ((uint64_t)(4 * (fold_mask + 1) * 2 + 3)) * (p->mod.m - 1) < (1ull << 32))
            fold_mask = fold_mask * 2 + 1;
        const unsigned grid = (unsigned)std::min<uint64_t>(p->ctx->n_cu * (uint64_t)REPLAY_WG_PER_CU,
                                                           ceil_div(max_units * n_chunks, 4));
        {
            KernelTimer kt(p->ctx, st, "replayable_sweep");
            hipLaunchKernelGGL(k_replayable_sweep_fast<REPLAY_U>, dim3(grid), dim3(256), 0, st, sc.b.units,
                               sc.b.n_units, sc.b.sorted_h0, p->d_table, E, p->d_classes, p->n_classes, p->mod.m,
                               p->mod.mu, p->mod.m_k64, REPLAY_EC, n_chunks, fold_mask, sc.counter,
                               d_partial, stride);
        }
        hipLaunchKernelGGL(k_replayable_merge<REPLAY_U>, dim3(ceil_div(max_units * per_unit, 256)), dim3(256), 0, st,
                           sc.b.units, sc.b.n_units, sc.b.sorted_idx, d_partial, stride, n_chunks,
                           d_stats);
    } else {
        KernelTimer kt(p->ctx, st, "replayable_sweep");
        const uint64_t units64 = S / 64 + 256;
        hipLaunchKernelGGL(k_replayable_sweep_general, dim3(ceil_div(units64, 4)), dim3(256), 0, st,
                           sc.b.units, sc.b.n_units, sc.b.sorted_h0, sc.b.sorted_idx, p->d_table, E,
                           p->d_classes, p->n_classes, p->mod.m, d_stats);
    }
    NMZ_HIP(hipGetLastError());
    return NMZ_OK;
}

}  // namespace nmz
