// K1 -- order-query statistics (replayablepolicy.go:100-114): the plan-side row images (oq_build) and the sweep
// kernel that answers each (seed, class segment) with block searches instead of per-event decisions (oq_sweep).
// replayable.hip explains the algebra this builds on (steps 1-4).
#include <algorithm>
#include <cstdlib>
#include <string>
#include <vector>

#include "nmz_common.h"
#include "nmz_internal.h"
#include "replayable_plan.h"

namespace nmz {

// ---------------------------------------------------------------------------
// Order-query statistics (0 < m < 2^32): the per-seed sum, max and first argmax of
// every decision of a (row L, class) segment without deciding event by event.
//
// Inside a segment (C-sorted) every decision is t = (base + Cm) mod m with
// base = Hm on the carry-free prefix [0, d) and Hm2 on [d, n). For a set of
// events with one base b:
//   sum t = |set| b + sum Cm - m #{Cm >= m - b}       (each t wraps at most once)
//   max t = b + max{Cm < m - b}   if that set is non-empty (those t lie in [b, m),
//           b + max Cm - m        otherwise              the wrapped ones in [0, b))
// so a block of events sorted by (Cm, e desc) answers both with one binary
// search for m - b: the count gives the wraps, the entry just below gives the
// maximum and its smallest e. The prefix/suffix split at d is covered by
// aligned blocks of three levels (512, 64, 8 events; each block sorted within
// itself), the 8-event block holding d is decided event by event (which also
// counts d exactly). Per (seed, segment of n events): n/512 + 16 block searches
// instead of n decisions. Segments of <= OQ_BRUTE events are decided event by
// event with wave-uniform table reads. The sum over all segments needs only the
// carry-free counts d and the wrap count W:
//   sum = sum_segments (d Hm + (n - d) Hm2) + sum_row Cm - m W.
//
// LDS image of a row (uint2 units): the three level arrays {Cm, ~e} and the 8-event samples of C, each
// segment's arrays skewed (logical entry i at base + i + i/32) so that the power-of-two strides of a
// binary search land on distinct banks; a block that the segment end cuts short is padded with copies of
// its last (largest) entry, so every search runs over a whole block with immediate-offset reads.
// ---------------------------------------------------------------------------
constexpr uint32_t OQ_S0 = 512, OQ_S1 = 64, OQ_S2 = 8;
constexpr uint32_t OQ_BRUTE = 64;   // segments of at most this many events: per-event decisions
constexpr uint32_t OQ_LDS_MAX = 160 * 1024;

__host__ __device__ constexpr uint32_t oq_skew(uint32_t i) { return i + (i >> 5); }
__host__ __device__ constexpr uint32_t oq_round(uint32_t n, uint32_t s) { return (n + s - 1) / s * s; }

struct OqClass {
    uint64_t pn;            // P^len
    uint32_t start, count;  // table segment (C order)
    uint32_t lv[3];         // level-array bases in the row image (uint2 units)
    uint32_t samp, samp_p2; // sample base; sample slots (a power of two >= ceil(n / 8))
    uint32_t pass;          // the pass (row image) holding this segment
    uint32_t pad[2];
};

// plan: one workgroup per (top block, row L): the top block's entries (C order) sorted by (Cm, ~e) with a
// bitonic network whose runs all end ascending after every stage (the first step of stage k compares an
// element with its mirror in the k-run), so the 8-, 64- and 512-runs are snapshots of the three levels.
// Also writes the 8-event samples of C and adds the block's C mod m to the row sum.
__global__ __launch_bounds__(256) void k_replayable_oq_levels(const uint4 *__restrict__ table, uint32_t E,
                                                              const uint4 *__restrict__ tb_list,
                                                              const OqClass *__restrict__ classes,
                                                              const uint4 *__restrict__ passes,
                                                              uint4 *__restrict__ blob,
                                                              unsigned long long *__restrict__ rowsum) {
    __shared__ uint64_t key[OQ_S0];
    __shared__ unsigned long long part[4];
    const uint4 tb = tb_list[blockIdx.x];  // {class, block start in the segment, size, 0}
    const OqClass ci = classes[tb.x];
    const uint4 ps = passes[ci.pass];      // {image offset lo, hi (uint4 units), rb16, 0}
    const uint32_t L = blockIdx.y, lo = tb.y, size = tb.z, n = ci.count;
    const bool levels = n > OQ_BRUTE;
    const uint4 *__restrict__ row = table + (uint64_t)L * E + ci.start + lo;
    uint2 *img = reinterpret_cast<uint2 *>(blob + ((uint64_t)ps.y << 32 | ps.x) + (uint64_t)L * ps.z);
    rowsum += 256 * ci.pass;
    uint64_t s = 0;
    for (uint32_t i = threadIdx.x; i < OQ_S0; i += 256) {
        if (i < size) {
            const uint4 q = row[i];
            key[i] = ((uint64_t)q.z << 32) | q.w;
            s += q.z;
            if (levels && (i & 7) == 0) img[ci.samp + oq_skew((lo + i) / 8)] = make_uint2(q.x, q.y);
        } else {
            key[i] = UINT64_MAX;
        }
    }
    if (levels && lo == 0)  // sample padding: above every ~H but ~0 (H = 0), where the count is clamped to ns
        for (uint32_t k = (n + 7) / 8 + threadIdx.x; k < ci.samp_p2; k += 256)
            img[ci.samp + oq_skew(k)] = make_uint2(~0u, ~0u);
    for (int o = 32; o; o >>= 1) s += __shfl_xor(s, o, 64);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) atomicAdd(rowsum + L, part[0] + part[1] + part[2] + part[3]);
    if (!levels) return;
    const uint32_t p = threadIdx.x;  // one compare-exchange pair per thread
    for (uint32_t k = 2; k <= OQ_S0; k <<= 1) {
        for (uint32_t j = k >> 1; j; j >>= 1) {
            uint32_t i, l;
            if (j == k >> 1) {  // mirror step
                i = (p / j) * k + (p % j);
                l = (p / j) * k + (k - 1 - (p % j));
            } else {
                i = (p / j) * 2 * j + (p % j);
                l = i + j;
            }
            const uint64_t a = key[i], b = key[l];
            if (a > b) {
                key[i] = b;
                key[l] = a;
            }
            __syncthreads();
        }
        const int lv = k == OQ_S2 ? 2 : k == OQ_S1 ? 1 : k == OQ_S0 ? 0 : -1;
        if (lv >= 0) {
            // the level's storage covers the segment rounded up to 512 (level 0) or 64 events
            const uint32_t padlen = oq_round(n, lv == 0 ? OQ_S0 : OQ_S1);
            for (uint32_t i = threadIdx.x; i < OQ_S0 && lo + i < padlen; i += 256) {
                const uint32_t b0 = i & ~(k - 1);
                const uint32_t last = b0 < size ? min(b0 + k, size) - 1 : size - 1;
                const uint64_t q = key[i < size ? i : last];
                const uint2 w = make_uint2((uint32_t)(q >> 32), (uint32_t)q);
                img[ci.lv[lv] + oq_skew(lo + i)] = w;
                // the skew slot after every 32 entries repeats the entry before it, so the entry below phys(idx)
                // is always at phys(idx) - 1
                if (((lo + i) & 31) == 31) img[ci.lv[lv] + oq_skew(lo + i) + 1] = w;
            }
            __syncthreads();
        }
    }
}

// one decision from a table entry {C lo, C hi, Cm, ~e}: counts carry-free events (d) and wraps (W).
// BIG: m >= 2^31, where base + Cm can overflow 32 bits (then the true sum exceeds m, and t = sum - m < m is exact
// modulo 2^32)
template <bool BIG>
__device__ __forceinline__ void oq_decide(uint4 q, uint64_t nH, uint32_t Hm, uint32_t Hm2, uint32_t m, uint32_t &d,
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

// phys offset (from phys(idx)) of element idx + s - 1 in a skewed block, idx a multiple of 2s; and the step
// of phys(idx) when idx grows by s
__host__ __device__ constexpr uint32_t oq_off(uint32_t s) { return s >= 32 ? s - 2 + s / 32 : s - 1; }
__host__ __device__ constexpr uint32_t oq_inc(uint32_t s) { return s >= 32 ? s + s / 32 : s; }

// Interleaved searches over whole sorted blocks (skewed, padded with copies of the block's largest entry):
// chains [0, N0) over 512-blocks, [N0, N0 + N1) over 64-blocks, the rest over 8-blocks, stepped together
// so that every chain ends in the same round (9 dependent rounds of independent LDS reads). Per chain:
// cnt = #{Cm < X} (0..S), cand = the entry just below X, or the block's largest entry when none is below X
// (wrap). pb = phys index of the block's first entry.
template <int N0, int N1, int N2>
__device__ __forceinline__ void oq_search(const uint2 *__restrict__ img, const uint32_t (&pb)[N0 + N1 + N2],
                                          const uint32_t (&X)[N0 + N1 + N2], uint32_t (&cnt)[N0 + N1 + N2],
                                          uint2 (&cand)[N0 + N1 + N2], bool (&wrap)[N0 + N1 + N2]) {
    constexpr int NC = N0 + N1 + N2;
    // byte addresses, so every step is one ds_read_b32 with an immediate offset
    const char *__restrict__ base = reinterpret_cast<const char *>(img);
    uint32_t Q[NC];
#pragma unroll
    for (int k = 0; k < NC; ++k) Q[k] = pb[k] * 8u;
#pragma unroll
    for (uint32_t r = 0; r < 9; ++r) {
#pragma unroll
        for (int k = 0; k < NC; ++k) {
            const uint32_t lg = k < N0 ? 8 : k < N0 + N1 ? 5 : 2;  // log2(S) - 1
            if (r + lg >= 8) {
                const uint32_t st = 1u << (8 - r);
                const uint32_t v = *reinterpret_cast<const uint32_t *>(base + Q[k] + 8u * oq_off(st));
                Q[k] = v < X[k] ? Q[k] + 8u * oq_inc(st) : Q[k];
            }
        }
    }
#pragma unroll
    for (int k = 0; k < NC; ++k) {
        const uint32_t S = k < N0 ? OQ_S0 : k < N0 + N1 ? OQ_S1 : OQ_S2;
        const uint2 first = *reinterpret_cast<const uint2 *>(base + pb[k] * 8u + 8u * oq_skew(S - 1));
        const uint32_t q = (Q[k] >> 3) - pb[k];
        const uint32_t idx = q - ((q * 993u) >> 15);  // phys -> logical (q = idx + idx/32 < 33 * 32)
        const uint2 c = *reinterpret_cast<const uint2 *>(base + Q[k] - 8u);  // idx - 1 (pad slots repeat it)
        const bool all = first.x < X[k];
        cnt[k] = all ? S : idx;
        wrap[k] = !all && idx == 0;
        cand[k] = (all || idx == 0) ? first : c;
        // finish four chains at a time: the compiler would otherwise issue every chain's two final reads
        // at once and spill
        if ((k & 3) == 3) asm volatile("" ::: "memory");
    }
}

// fold one block result into the seed's statistics; side 0 = not this lane's block, 1 = carry-free (Hm),
// 2 = carry (Hm2); rs = the block's real size
__device__ __forceinline__ void oq_accum(int side, uint32_t rs, uint32_t cnt, uint2 cand, bool wrap, uint32_t Hm,
                                         uint32_t Hm2, uint32_t m, uint32_t &W, uint64_t &key) {
    const uint32_t b = side == 2 ? Hm2 : Hm;
    const uint32_t t = b + cand.x - (wrap ? m : 0u);
    const uint64_t k = side ? (((uint64_t)t << 32) | cand.y) : 0ull;
    W += side ? rs - min(cnt, rs) : 0u;
    key = k > key ? k : key;
}

// One seed's statistics over one class segment (replayablepolicy.go:100-114 restated per segment, see above):
// adds d Hm + (n - d) Hm2 to sum, the segment's wraps to W, and folds its maximum key {t, ~e} into key.
// BIG: 2^31 <= m < 2^32 (block results need no change: t = b + Cm - wrap * m is exact modulo 2^32).
template <bool BIG>
__device__ __forceinline__ void oq_seed_class(const OqClass &ci, const uint2 *__restrict__ img,
                                              const uint4 *__restrict__ row, uint64_t h0, uint32_t m, uint64_t mu,
                                              uint32_t m_k64, uint64_t &sum, uint32_t &W, uint64_t &key) {
    const uint32_t n = ci.count, cs = ci.start;
    const uint64_t H = h0 * ci.pn;
    const uint64_t nH = ~H;
    // Hm = H mod m; Hm2 = (Hm + 2^64 mod m) mod m, where for m >= 2^31 the 32-bit add may overflow (then the true
    // value exceeds m and one subtract, modulo 2^32, is exact)
    const uint32_t Hm = BIG ? mod_barrett64(H, m, mu) : mod_barrett_small(H, m, mu);
    const uint32_t t2 = Hm + m_k64;
    const uint32_t Hm2 = BIG ? ((t2 < Hm || t2 >= m) ? t2 - m : t2) : min(t2, t2 - m);
    uint32_t d = 0;
    if (n <= OQ_BRUTE) {
        for (uint32_t i = 0; i < n; ++i) oq_decide<BIG>(row[cs + i], nH, Hm, Hm2, m, d, W, key);
    } else {
        const uint32_t XA = m - Hm, XB = m - Hm2;
        const uint32_t ns = (n + 7) >> 3, nt = (n + OQ_S0 - 1) / OQ_S0;
        // 8-event blocks whose first C is <= ~H are carry-free up to that entry: binary search over the
        // samples (the C of every 8th entry, ascending; slots past ns hold whatever, so the count is clamped)
        uint32_t ks;
        {
            const uint32_t sb = ci.samp;
            uint32_t Q = sb;
            for (uint32_t st = ci.samp_p2 >> 1; st; st >>= 1) {
                const uint2 v = img[Q + oq_off(st)];
                Q = ((((uint64_t)v.y) << 32) | v.x) <= nH ? Q + oq_inc(st) : Q;
            }
            const uint32_t q = Q - sb;
            const uint32_t k0 = q - ((q * 993u) >> 15);
            const uint2 v = img[Q];  // the last slot the lifting cannot reach
            ks = min(k0 + (((((uint64_t)v.y) << 32) | v.x) <= nH ? 1u : 0u), ns);
        }
        const uint32_t b8 = ks ? 8 * (ks - 1) : 0;  // the 8-block holding the carry boundary
        const uint32_t be = b8 + 8;
        {
            const uint32_t nb = min(8u, n - b8);
            // decided event by event; the eight loads are issued together and the updates are selects (a
            // guarded update had let the compiler sink each load into its own branch and wait for it there)
            uint4 q[8];
#pragma unroll
            for (uint32_t i = 0; i < 8; ++i) q[i] = row[cs + b8 + min(i, nb - 1)];
#pragma unroll
            for (uint32_t i = 0; i < 8; ++i) {
                uint32_t dd = 0, ww = 0;
                uint64_t kk = 0;
                oq_decide<BIG>(q[i], nH, Hm, Hm2, m, dd, ww, kk);
                const bool in = i < nb;
                d += in ? dd : 0u;
                W += in ? ww : 0u;
                key = (in && kk > key) ? kk : key;
            }
        }
        d += b8;
        const uint32_t pad1 = oq_round(n, OQ_S1);
        // level 0: every 512-block of the segment, two at a time (this lane's boundary block is searched
        // and dropped)
        for (uint32_t b = 0; b < nt; b += 2) {
            uint32_t pb[2], X[2], cn[2];
            uint2 cand[2];
            bool wr[2];
            int side[2];
            uint32_t rs[2];
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const uint32_t lo = min(b + k, nt - 1) * OQ_S0, hi = min(lo + OQ_S0, n);
                side[k] = b + k >= nt ? 0 : hi <= b8 ? 1 : lo >= be ? 2 : 0;
                X[k] = side[k] == 2 ? XB : XA;
                pb[k] = ci.lv[0] + oq_skew(lo);
                rs[k] = hi - lo;
            }
            if (__builtin_amdgcn_ballot_w64(side[0] != 0 || side[1] != 0)) {  // n <= 512: boundary only
                oq_search<2, 0, 0>(img, pb, X, cn, cand, wr);
#pragma unroll
                for (int k = 0; k < 2; ++k) oq_accum(side[k], rs[k], cn[k], cand[k], wr[k], Hm, Hm2, m, W, key);
            }
        }
#pragma unroll
        for (int h = 0; h < 2; ++h) {  // level 1: the eight 64-blocks of the boundary 512-block, 4 at a time
            const uint32_t lt = (b8 & ~(OQ_S0 - 1)) + h * 4 * OQ_S1;
            uint32_t pb[4], X[4], cn[4], rs[4];
            int side[4];
            uint2 cand[4];
            bool wr[4], any = false;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const uint32_t lo = lt + k * OQ_S1, hi = min(lo + OQ_S1, n);
                side[k] = lo >= n ? 0 : hi <= b8 ? 1 : lo >= be ? 2 : 0;
                any |= side[k] != 0;
                X[k] = side[k] == 2 ? XB : XA;
                pb[k] = ci.lv[1] + oq_skew(min(lo, pad1 - OQ_S1));
                rs[k] = hi - lo;
            }
            if (__builtin_amdgcn_ballot_w64(any)) {
                oq_search<0, 4, 0>(img, pb, X, cn, cand, wr);
#pragma unroll
                for (int k = 0; k < 4; ++k) oq_accum(side[k], rs[k], cn[k], cand[k], wr[k], Hm, Hm2, m, W, key);
            }
        }
#pragma unroll
        for (int h = 0; h < 2; ++h) {  // level 2: the 8-blocks of the boundary 64-block, less the one decided above
            const uint32_t lm = (b8 & ~(OQ_S1 - 1)) + h * 4 * OQ_S2;
            uint32_t pb[4], X[4], cn[4], rs[4];
            int side[4];
            uint2 cand[4];
            bool wr[4], any = false;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const uint32_t lo = lm + k * OQ_S2, hi = min(lo + OQ_S2, n);
                side[k] = (lo >= n || lo == b8) ? 0 : lo < b8 ? 1 : 2;
                any |= side[k] != 0;
                X[k] = side[k] == 2 ? XB : XA;
                pb[k] = ci.lv[2] + oq_skew(min(lo, pad1 - OQ_S2));
                rs[k] = hi - lo;
            }
            if (__builtin_amdgcn_ballot_w64(any)) {
                oq_search<0, 0, 4>(img, pb, X, cn, cand, wr);
#pragma unroll
                for (int k = 0; k < 4; ++k) oq_accum(side[k], rs[k], cn[k], cand[k], wr[k], Hm, Hm2, m, W, key);
            }
        }
    }
    sum += (uint64_t)d * Hm + (uint64_t)(n - d) * Hm2;
}

// ACC: a later pass over other class segments of the row -- combine with the statistics of the earlier passes
template <bool ACC>
__device__ __forceinline__ void oq_store(nmz_sched_stats *__restrict__ stats, uint32_t idx, uint64_t sum,
                                         uint64_t key) {
    if constexpr (ACC) {
        const nmz_sched_stats o = stats[idx];
        sum += o.sum_delay_ns;
        const uint64_t ko = ((uint64_t)o.max_delay_ns << 32) | (uint32_t)~o.argmax_event;
        key = ko > key ? ko : key;
    }
    nmz_sched_stats st;
    st.sum_delay_ns = sum;
    st.max_delay_ns = (int64_t)(key >> 32);
    st.argmax_event = ~(uint32_t)key;
    st.n_fault = 0;
    st.first_fault = NMZ_NONE;
    st.flags = 0;
    stats[idx] = st;
}

#ifdef OQ_TRACE
// debug builds only (-DOQ_TRACE): wall_clock64 per (row, wave) at the kernel start [9], after staging [0], at the
// end of each of up to 7 seed chunks [1..7] and after the cooperative tail [8]; read with nmz_debug_oq_trace
__device__ unsigned long long g_oq_trace[256][16][10];
#endif

// One workgroup per row L (256 workgroups, one per CU): the row image is staged into LDS once, then the 16
// waves take the row's seeds in chunks of 64 from an LDS counter. A chunk is a chain of dependent LDS searches
// (~19 us for a wave alone, 20-45 us beside 15 others): with a fixed share of chunks per wave the row waited
// for the waves the SIMD arbiter served last (a row of 4 chunks per wave ended at ~140 us with its median wave
// done at ~110). The row's last partial chunk (ns % 64 seeds) is shared by the waves as they finish: each
// takes a subset of its class segments, and the partial statistics meet in LDS (u64 add and max are
// associative), so it costs about one class chain instead of a whole chunk.
constexpr uint32_t OQ_TAIL = 64;
constexpr uint32_t OQ_TAIL_LDS = OQ_TAIL * 16 + 16;  // {sum, key} per tail seed + the chunk counter

template <bool BIG, bool ACC>
__global__ __launch_bounds__(OQ_WG) void k_replayable_sweep_oq(
    const uint32_t *__restrict__ bucket_off, const uint64_t *__restrict__ sorted_h0,
    const uint32_t *__restrict__ sorted_idx, const uint4 *__restrict__ table, uint32_t E,
    const uint4 *__restrict__ blob, uint32_t rb16, const unsigned long long *__restrict__ rowsum,
    const OqClass *__restrict__ classes, uint32_t n_classes, uint32_t m, uint64_t mu, uint32_t m_k64,
    nmz_sched_stats *__restrict__ stats, unsigned long long *__restrict__ span) {
    extern __shared__ uint4 oq_lds[];
    const uint32_t L = blockIdx.x;
    const uint32_t s0 = bucket_off[L], s1 = bucket_off[L + 1];
    if (s0 == s1) return;
    if (span && threadIdx.x == 0) atomicMax(span, ~(unsigned long long)wall_clock64());
#ifdef OQ_TRACE
    if ((threadIdx.x & 63) == 0) {
        for (int k = 0; k < 10; ++k) g_oq_trace[L][threadIdx.x >> 6][k] = 0;
        g_oq_trace[L][threadIdx.x >> 6][9] = wall_clock64();
    }
#endif
    const uint32_t ns_row = s1 - s0;
    const uint32_t rem = ns_row % 64;
    const uint32_t tail = rem;  // the partial chunk, shared by all waves
    const uint32_t smain = s1 - tail, nch = (smain - s0) / 64;
    unsigned long long *tacc = reinterpret_cast<unsigned long long *>(oq_lds + rb16);  // [OQ_TAIL][2]
    uint32_t *ctr = reinterpret_cast<uint32_t *>(tacc + 2 * OQ_TAIL);
    {
        const uint4 *__restrict__ src = blob + (uint64_t)L * rb16;
        // every load of a pass in flight at once: loads and stores unconditional, indices clamped to the image
        // (guarded loads had compiled to one wait per load plus scratch copies)
        constexpr uint32_t B = 8;  // 128 KB per pass
        for (uint32_t i0 = 0; i0 < rb16; i0 += B * OQ_WG) {
            uint4 v[B];
#pragma unroll
            for (uint32_t k = 0; k < B; ++k) v[k] = src[min(i0 + k * OQ_WG + threadIdx.x, rb16 - 1)];
            // the clamped slots all write the image's last entry to its own place
#pragma unroll
            for (uint32_t k = 0; k < B; ++k) oq_lds[min(i0 + k * OQ_WG + threadIdx.x, rb16 - 1)] = v[k];
        }
        if (tail)
            for (uint32_t i = threadIdx.x; i < 2 * OQ_TAIL; i += OQ_WG) tacc[i] = 0;
        if (threadIdx.x == 0) *ctr = 0;
    }
    __syncthreads();
#ifdef OQ_TRACE
    uint32_t tr_n = 0;
    if ((threadIdx.x & 63) == 0) g_oq_trace[L][threadIdx.x >> 6][tr_n] = wall_clock64();
    ++tr_n;
#endif
    const uint2 *img = reinterpret_cast<const uint2 *>(oq_lds);
    const uint4 *__restrict__ row = table + (uint64_t)L * E;
    const uint64_t rsum = rowsum[L];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (;;) {
        uint32_t ch = 0;
        if (lane == 0) ch = atomicAdd(ctr, 1u);
        ch = __builtin_amdgcn_readfirstlane(ch);
        if (ch >= nch) break;
        const uint32_t j = s0 + ch * 64 + lane;
        const uint64_t h0 = sorted_h0[j];
        uint64_t sum = 0, key = 0;
        uint32_t W = 0;
        for (uint32_t c = 0; c < n_classes; ++c) {
            const OqClass ci = classes[c];
            oq_seed_class<BIG>(ci, img, row, h0, m, mu, m_k64, sum, W, key);
        }
        oq_store<ACC>(stats, sorted_idx[j], sum + rsum - (uint64_t)W * m, key);
#ifdef OQ_TRACE
        if (lane == 0 && tr_n < 8) g_oq_trace[L][wave][tr_n] = wall_clock64();
        ++tr_n;
#endif
    }
    if (tail) {
        // r chunks of <= 64 tail seeds; wave w takes chunk w % r and every P-th class segment from w / r
        const uint32_t r = (tail + 63) >> 6, P = (OQ_WG / 64) / r;
        if (wave < r * P) {
            const uint32_t jj = (wave % r) * 64 + lane, part = wave / r;
            const uint64_t h0 = sorted_h0[smain + min(jj, tail - 1)];
            uint64_t sum = 0, key = 0;
            uint32_t W = 0;
            for (uint32_t c = part; c < n_classes; c += P) {
                const OqClass ci = classes[c];
                oq_seed_class<BIG>(ci, img, row, h0, m, mu, m_k64, sum, W, key);
            }
            if (jj < tail) {
                atomicAdd(tacc + 2 * jj, (unsigned long long)(sum - (uint64_t)W * m));
                atomicMax(tacc + 2 * jj + 1, (unsigned long long)key);
            }
        }
        __syncthreads();
        if (threadIdx.x < tail)
            oq_store<ACC>(stats, sorted_idx[smain + threadIdx.x], tacc[2 * threadIdx.x] + rsum,
                          tacc[2 * threadIdx.x + 1]);
#ifdef OQ_TRACE
        if (lane == 0) g_oq_trace[L][wave][8] = wall_clock64();
#endif
    }
    if (span) {  // one atomic per workgroup: 4,096 same-address atomics at once (one per wave) queue for ~35 us
        __syncthreads();
        if (threadIdx.x == 0) atomicMax(span + 1, (unsigned long long)wall_clock64());
    }
}

// read at every call (free without NMZ_AB=1), so a test can switch it inside one process
bool replay_oq_enabled() {
    const char *e = ab_env("NMZ_REPLAY_OQ");
    return !(e && std::string(e) == "0");
}

// image size (uint2 units, before the region offsets) of one class segment's order-query arrays
struct OqLen {
    uint64_t v[4] = {0, 0, 0, 0};  // level 0, 1, 2 and samples
};
static OqLen oq_seg_len(uint32_t n) {
    OqLen l;
    if (n > OQ_BRUTE) {
        l.v[0] = oq_skew(oq_round(n, OQ_S0));
        l.v[1] = l.v[2] = oq_skew(oq_round(n, OQ_S1));
        uint32_t p2 = 1;
        while (p2 < (n + 7) / 8) p2 <<= 1;
        l.v[3] = oq_skew(p2);
    }
    return l;
}
static uint64_t oq_image_bytes(const uint64_t (&len)[4]) {
    return ((len[0] + len[1] + len[2] + len[3]) * 8 + 15) & ~15ull;
}

// Build the order-query row images after the C sort (0 < m < 2^32). A row image that fits one workgroup's LDS
// is one pass over the length classes (configs[1]: 110 KB at E = 4,096). A longer trace splits its classes into
// C-sorted sub-segments of at most OQ_SUBSEG events -- each one is a segment in its own right: every decision of
// it is (base + Cm) mod m with the same carry rule (C > ~H), just over fewer events -- and packs them into passes
// whose images fit; the kernel runs once per pass and combines the passes' statistics per seed.
constexpr uint32_t OQ_SUBSEG = 4096;
int oq_build(OqState &o, const uint4 *d_table, uint32_t E, const ModParams &mod, const std::vector<ClassInfo> &cls,
             hipStream_t st) {
    o.on = false;
    o.passes.clear();
    if (!mod.m32ok || E == 0) return NMZ_OK;
    uint64_t budget = OQ_LDS_MAX - OQ_TAIL_LDS;
    if (const char *e = ab_env("NMZ_REPLAY_OQ_BUDGET"))  // tests: force several passes on short traces
        budget = std::min<uint64_t>(budget, std::max<uint64_t>(4096, strtoull(e, nullptr, 10)));
    // segments: the classes whole when the whole row fits one pass, else sub-segments of <= OQ_SUBSEG events
    std::vector<ClassInfo> seg;
    {
        uint64_t len[4] = {1, 0, 0, 0};
        for (const ClassInfo &c : cls) {
            const OqLen l = oq_seg_len(c.count);
            for (int r = 0; r < 4; ++r) len[r] += l.v[r];
        }
        const bool split = oq_image_bytes(len) > budget;
        // sub-segments small enough that one always fits the budget
        uint32_t sub = OQ_SUBSEG;
        while (sub > OQ_S0) {
            const OqLen l = oq_seg_len(sub);
            const uint64_t one[4] = {1 + l.v[0], l.v[1], l.v[2], l.v[3]};
            if (oq_image_bytes(one) <= budget) break;
            sub /= 2;
        }
        for (const ClassInfo &c : cls) {
            if (!split || c.count <= sub) {
                seg.push_back(c);
                continue;
            }
            for (uint32_t lo = 0; lo < c.count; lo += sub)
                seg.push_back(ClassInfo{c.pn, c.start + lo, std::min(sub, c.count - lo)});
        }
    }
    // passes: consecutive segments while the image fits (slot 0 of every image stays free, so the read below a
    // block, unused when the count is 0, never leaves the image)
    std::vector<OqClass> oc(seg.size());
    std::vector<uint4> tbl;
    uint64_t off16 = 0;
    for (size_t c0 = 0; c0 < seg.size();) {
        uint64_t len[4] = {1, 0, 0, 0};
        size_t c1 = c0;
        for (; c1 < seg.size(); ++c1) {
            const OqLen l = oq_seg_len(seg[c1].count);
            uint64_t t[4];
            for (int r = 0; r < 4; ++r) t[r] = len[r] + l.v[r];
            if (c1 > c0 && oq_image_bytes(t) > budget) break;
            OqClass &q = oc[c1];
            q = OqClass{};
            q.pn = seg[c1].pn;
            q.start = seg[c1].start;
            q.count = seg[c1].count;
            q.pass = (uint32_t)o.passes.size();
            if (q.count > OQ_BRUTE) {
                q.lv[0] = (uint32_t)len[0];
                q.lv[1] = (uint32_t)len[1];
                q.lv[2] = (uint32_t)len[2];
                q.samp = (uint32_t)len[3];
                uint32_t p2 = 1;
                while (p2 < (q.count + 7) / 8) p2 <<= 1;
                q.samp_p2 = p2;
            }
            for (int r = 0; r < 4; ++r) len[r] = t[r];
            for (uint32_t lo = 0; lo < q.count; lo += OQ_S0)
                tbl.push_back(make_uint4((uint32_t)c1, lo, std::min(OQ_S0, q.count - lo), 0));
        }
        const uint64_t rb = oq_image_bytes(len);
        if (rb > budget) return NMZ_OK;  // cannot happen with OQ_SUBSEG segments; keep the per-decision sweep
        for (size_t c = c0; c < c1; ++c) {  // regions: level 0 | level 1 | level 2 | samples
            oc[c].lv[1] += (uint32_t)len[0];
            oc[c].lv[2] += (uint32_t)(len[0] + len[1]);
            oc[c].samp += (uint32_t)(len[0] + len[1] + len[2]);
        }
        o.passes.push_back(OqState::Pass{(uint32_t)c0, (uint32_t)c1, off16, (uint32_t)(rb / 16)});
        off16 += 256 * (rb / 16);
        c0 = c1;
    }
    // function attributes are per device, and contexts on several devices (or threads) build plans
    // concurrently: set them on every build (cheap) instead of behind a process-wide flag
    for (const void *f : {reinterpret_cast<const void *>(k_replayable_sweep_oq<false, false>),
                          reinterpret_cast<const void *>(k_replayable_sweep_oq<false, true>),
                          reinterpret_cast<const void *>(k_replayable_sweep_oq<true, false>),
                          reinterpret_cast<const void *>(k_replayable_sweep_oq<true, true>)})
        if (hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)OQ_LDS_MAX) != hipSuccess) {
            o.passes.clear();
            return NMZ_OK;  // keep the per-decision sweep
        }
    const size_t np = o.passes.size();
    std::vector<uint4> passes(np);
    for (size_t i = 0; i < np; ++i)
        passes[i] = make_uint4((uint32_t)o.passes[i].off16, (uint32_t)(o.passes[i].off16 >> 32), o.passes[i].rb16, 0);
    uint4 *d_tbl, *d_passes;
    ScratchLayout lay;
    lay.add(&o.d_blob, off16).add(&o.d_rowsum, 256 * np).add(&o.d_classes, oc.size()).add(&d_tbl, tbl.size());
    lay.add(&d_passes, np);
    NMZ_TRY(lay.bind(o.mem));
    NMZ_HIP(hipMemsetAsync(o.d_blob, 0, off16 * 16, st));
    NMZ_HIP(hipMemsetAsync(o.d_rowsum, 0, 256 * np * 8, st));
    NMZ_TRY(copy_h2d(o.d_classes, oc.data(), oc.size(), st));
    NMZ_TRY(copy_h2d(d_tbl, tbl.data(), tbl.size(), st));
    NMZ_TRY(copy_h2d(d_passes, passes.data(), np, st));
    hipLaunchKernelGGL(k_replayable_oq_levels, dim3((unsigned)tbl.size(), 256), dim3(256), 0, st, d_table, E, d_tbl,
                       o.d_classes, d_passes, o.d_blob, reinterpret_cast<unsigned long long *>(o.d_rowsum));
    NMZ_HIP(hipGetLastError());
    NMZ_HIP(hipStreamSynchronize(st));  // the host vectors above are pageable
    o.on = true;
    return NMZ_OK;
}

int oq_sweep(const OqState &o, nmz_ctx *ctx, hipStream_t st, const Buckets &b, const uint4 *d_table, uint32_t E,
             const ModParams &mod, nmz_sched_stats *d_stats) {
    KernelTimer kt(ctx, st, "replayable_sweep");
    unsigned long long *span = kt.span();
    const bool big = mod.m32 >= 0x80000000u;
    for (size_t i = 0; i < o.passes.size(); ++i) {
        const OqState::Pass &ps = o.passes[i];
        auto kern = big ? (i ? k_replayable_sweep_oq<true, true> : k_replayable_sweep_oq<true, false>)
                        : (i ? k_replayable_sweep_oq<false, true> : k_replayable_sweep_oq<false, false>);
        hipLaunchKernelGGL(kern, dim3(256), dim3(OQ_WG), ps.rb16 * 16u + OQ_TAIL_LDS, st, b.offset, b.sorted_h0,
                           b.sorted_idx, d_table, E, o.d_blob + ps.off16, ps.rb16,
                           reinterpret_cast<const unsigned long long *>(o.d_rowsum + 256 * i),
                           o.d_classes + ps.c0, ps.c1 - ps.c0, mod.m32, mod.mu, mod.m_k64, d_stats, span);
    }
    NMZ_HIP(hipGetLastError());
    return NMZ_OK;
}

}  // namespace nmz

#ifdef OQ_TRACE
extern "C" int nmz_debug_oq_trace(unsigned long long *out) {
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(nmz::g_oq_trace), sizeof(nmz::g_oq_trace)) == hipSuccess ? 0 : -1;
}
#endif
