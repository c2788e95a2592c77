// K1 -- the wavelet-tree plan: the row images the sweep of replayable_wt.hip stages into LDS (that file's header
// explains the algebra and what the image holds). wt_layout decides whether the images apply and lays out the
// segments, k_replayable_wt_build builds them, one workgroup per (segment, row L); wt_launch and wt_build run it.
#include <algorithm>
#include <cstring>
#include <numeric>
#include <cstdlib>
#include <string>
#include <vector>

#include "nmz_common.h"
#include "nmz_internal.h"
#include "replayable_plan.h"
#include "replayable_wt_dev.h"

namespace nmz {

#ifdef WT_BUILD_TRACE
// timing-only builds: wall_clock64() at the plan kernel's phase boundaries, per workgroup (tools/wt_build_trace.py)
constexpr uint32_t WT_TRACE_PHASES = 10, WT_TRACE_WGS = 8192;
__device__ unsigned long long g_wt_build_trace[WT_TRACE_WGS * WT_TRACE_PHASES];
#define WT_STAMP(k)                                                                                              \
    do {                                                                                                         \
        if (threadIdx.x == 0 && blockIdx.y * gridDim.x + blockIdx.x < WT_TRACE_WGS)                              \
            g_wt_build_trace[(L * gridDim.x + c) * WT_TRACE_PHASES + (k)] = wall_clock64();                      \
    } while (0)
#else
#define WT_STAMP(k) \
    do {            \
    } while (0)
#endif

// WtClass (the segment descriptor) is in replayable_plan.h: the plan's host code packs it with the plan's inputs

// ---------------------------------------------------------------------------------------------------------------
// plan: one workgroup per (segment, row L). Sorts the segment's keys (Cm << 32 | (0xffff - e) << 16 | position)
// in LDS (bitonic), writes Cm / e by rank and C_hi by position, the two bucket indexes, and the K wavelet levels:
// level l holds bit K-1-l of the ranks, in the order "stably sorted by the top l bits" (the node of the value
// prefix pi starts at pi << (K-l), since the ranks are a permutation of [0, n)), one {32 bits, ones before} pair
// per 32 positions. Also adds the segment's sum of Cm to the row sum (every segment, short ones included).
// ---------------------------------------------------------------------------------------------------------------
constexpr uint32_t WT_BT = 512, WT_BW = WT_BT / 64;  // plan kernel: threads and waves per workgroup

// The plan kernel's dynamic LDS (~75 KB, two workgroups per CU) as byte offsets, for the kernel's pointers and the
// launch's size alike: the keys, then (after the sort) the rank arrays in their place; the sorted keys; bucket
// counts (np / 2 buckets); level words and counts; small scratch
struct WtBuildLds {
    static constexpr uint32_t key = 0;                                 // u64 [WT_NMAX]; u16 [2][WT_NMAX] after the sort
    static constexpr uint32_t srt = key + WT_NMAX * 8;                 // u64 [WT_NMAX] sorted keys
    static constexpr uint32_t bc = srt + WT_NMAX * 8;                  // u32 [WT_NMAX / 2]
    static constexpr uint32_t wb = bc + WT_NMAX / 2 * 4;               // u32 [WT_NMAX / 32 + 4]
    static constexpr uint32_t cum = wb + (WT_NMAX / 32 + 4) * 4;       // u32 [WT_NMAX / 32 + 4]
    static constexpr uint32_t idx = cum + (WT_NMAX / 32 + 4) * 4;      // u32 [2][260] bucket indexes
    static constexpr uint32_t part = idx + 520 * 4;                    // u64 [WT_BW]
    static constexpr uint32_t bmax = part + WT_BW * 8;                 // u32 [4]
    static constexpr uint32_t total = bmax + 4 * 4;                    // the launch's dynamic LDS bytes
};
static_assert(WtBuildLds::total == 76944 && WtBuildLds::srt % 8 == 0 && WtBuildLds::part % 8 == 0,
              "the plan kernel's LDS carve");

// exclusive scan in place over nb <= 2,048 bucket counts (4 per thread, wave scans, then the wave totals in cum);
// *big gets the largest count above 32 (a bucket the per-bucket insertion sort should not take)
__device__ __forceinline__ void wt_bucket_scan(uint32_t *bc, uint32_t nb, uint32_t *cum, uint32_t *big, uint32_t tid) {
    const uint32_t lane = tid & 63, wave = tid >> 6, b0 = 4 * tid;
    uint32_t c4[4], t = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        c4[k] = b0 + k < nb ? bc[b0 + k] : 0u;
        t += c4[k];
        if (c4[k] > 32) atomicMax(big, c4[k]);
    }
    uint32_t inc = t;
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t v = __shfl_up(inc, o, 64);
        if (lane >= (uint32_t)o) inc += v;
    }
    if (lane == 63) cum[wave] = inc;
    __syncthreads();
    uint32_t base = inc - t;
    for (uint32_t w = 0; w < wave; ++w) base += cum[w];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (b0 + k < nb) bc[b0 + k] = base;  // bucket start (a cursor while scattering, then the end)
        base += c4[k];
    }
    __syncthreads();
}

// the plan's hints on the device, for the fused plan kernel (it computes and C-sorts its own table segments)
struct WtHints {
    const uint32_t *hoff;   // [E + 1] hint byte offsets (original event order)
    const uint8_t *hbytes;
    const uint32_t *perm;   // [E] length-sorted position -> event
    uint64_t m;             // the modulus (< 2^32 on this path) and floor(2^64 / m)
    uint64_t mu;
    uint4 *table;           // [256][E] out: {C lo, C hi, C mod m, ~e}, C-sorted per segment
    uint32_t *zero0;        // ranges the first workgroup zeroes (the plan's seed-scratch counters)
    uint32_t n_zero0;
    uint32_t *zero1;
    uint32_t n_zero1;
};

template <bool FUSED, int BB>
__global__ __launch_bounds__(WT_BT) void k_replayable_wt_build(const uint4 *__restrict__ table, uint32_t E,
                                                               WtClass *__restrict__ classes, uint32_t msh,
                                                               uint32_t mbits, uint4 *__restrict__ blob, uint32_t rb16,
                                                               unsigned long long *__restrict__ rowsum, WtHints hz) {
    extern __shared__ uint4 wt_build_lds[];
    char *lds = reinterpret_cast<char *>(wt_build_lds);
    uint64_t *key = reinterpret_cast<uint64_t *>(lds + WtBuildLds::key);
    uint16_t *S0 = reinterpret_cast<uint16_t *>(key);  // [2][WT_NMAX], after the sort
    uint64_t *srt = reinterpret_cast<uint64_t *>(lds + WtBuildLds::srt);
    uint32_t *bc = reinterpret_cast<uint32_t *>(lds + WtBuildLds::bc);
    uint32_t *cum = reinterpret_cast<uint32_t *>(lds + WtBuildLds::cum);
    uint32_t *idx = reinterpret_cast<uint32_t *>(lds + WtBuildLds::idx);
    unsigned long long *part = reinterpret_cast<unsigned long long *>(lds + WtBuildLds::part);
    uint32_t *bmax = reinterpret_cast<uint32_t *>(lds + WtBuildLds::bmax);
    // workgroups start in dispatch order (x fastest): the largest segments' rows first, so the small segments'
    // short workgroups fill in behind them instead of holding slots the large ones wait for
    const uint32_t lin = blockIdx.y * gridDim.x + blockIdx.x, L = lin & 255u;
    const uint32_t c = classes[lin >> 8].order, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    WT_STAMP(0);
    const WtClass ci = classes[c];
    const uint32_t n = ci.n;
    uint32_t np = 1, lgp = 0;
    while (np < n) {
        np <<= 1;
        ++lgp;
    }
    const uint32_t nb = np >= 2 ? np / 2 : 1, lgb = lgp ? lgp - 1 : 0;  // sort buckets (~2 keys each) and their bits
    if (tid < 4) bmax[tid] = 0;
    char *img = reinterpret_cast<char *>(blob + (uint64_t)L * rb16);
    // the segment's entries, one load each (every load in flight): the row sum, C's high words and the sort keys
    constexpr uint32_t PPT = WT_NMAX / WT_BT;
    uint4 q[PPT];
    if constexpr (FUSED) {
        if (lin == 0) {
            for (uint32_t i = tid; i < hz.n_zero0; i += WT_BT) hz.zero0[i] = 0;
            for (uint32_t i = tid; i < hz.n_zero1; i += WT_BT) hz.zero1[i] = 0;
        }
        // C = FNV-1a(seed bytes L, hint) - L * P^len (the table's correction, k_replayable_table) for the segment's
        // events, a thread per event and all of a thread's events in step (one hint length per segment), then
        // the stable C order through LDS: a counting sort on C's top bits and an insertion sort per bucket, or a
        // bitonic sort of (C, position) when a bucket holds more than 32 (repeated hints)
        uint16_t *posL = reinterpret_cast<uint16_t *>(key);  // [WT_NMAX] the sorted order's positions
        uint16_t *eL = posL + WT_NMAX;                       // [WT_NMAX] event by position (E <= 65,536)
        uint64_t h[PPT];
        uint32_t b0[PPT];
        uint32_t len = 0;
#pragma unroll
        for (uint32_t k = 0; k < PPT; ++k) {
            const uint32_t i = tid + k * WT_BT;
            h[k] = L;
            b0[k] = 0;
            if (i < n) {
                const uint32_t e = hz.perm[ci.start + i];
                eL[i] = (uint16_t)e;
                b0[k] = hz.hoff[e];
                len = hz.hoff[e + 1] - b0[k];
            }
        }
        len = __builtin_amdgcn_readfirstlane(len);  // lane 0 holds an event of the segment (n >= 1)
        // 16 hint bytes per round: the 5 aligned words covering them, all rounds' loads in flight together, then
        // v_alignbit to the hint's own byte order
        const uint32_t *__restrict__ hw = reinterpret_cast<const uint32_t *>(hz.hbytes);
        for (uint32_t c0 = 0; c0 < len; c0 += 16) {
            uint32_t w[PPT][5];
#pragma unroll
            for (uint32_t k = 0; k < PPT; ++k) {
                const uint32_t a = (b0[k] + c0) >> 2, wl = (b0[k] + len - 1) >> 2;
#pragma unroll
                for (uint32_t j = 0; j < 5; ++j) w[k][j] = tid + k * WT_BT < n ? hw[min(a + j, wl)] : 0u;
            }
#pragma unroll
            for (uint32_t k = 0; k < PPT; ++k) {
                const uint32_t sh = 8 * (b0[k] & 3);
                uint32_t u[4];
#pragma unroll
                for (uint32_t j = 0; j < 4; ++j) u[j] = __builtin_amdgcn_alignbit(w[k][j + 1], w[k][j], sh);
#pragma unroll
                for (uint32_t b = 0; b < 16; ++b)
                    if (c0 + b < len) h[k] = fnv_step(h[k], (u[b >> 2] >> (8 * (b & 3))) & 0xffu);
            }
        }
        const uint32_t shc = 64 - lgb;
        auto cb = [&](uint64_t C) { return lgb ? (uint32_t)(C >> shc) : 0u; };
        for (uint32_t b = tid; b < nb; b += WT_BT) bc[b] = 0;
        __syncthreads();
#pragma unroll
        for (uint32_t k = 0; k < PPT; ++k) {
            h[k] -= (uint64_t)L * ci.pn;  // C
            if (tid + k * WT_BT < n) atomicAdd(&bc[cb(h[k])], 1u);
        }
        __syncthreads();
        wt_bucket_scan(bc, nb, cum, bmax + 1, tid);
        if (bmax[1] == 0) {
#pragma unroll
            for (uint32_t k = 0; k < PPT; ++k) {
                const uint32_t i = tid + k * WT_BT;
                if (i < n) {
                    const uint32_t slot = atomicAdd(&bc[cb(h[k])], 1u);
                    srt[slot] = h[k];
                    posL[slot] = (uint16_t)i;
                }
            }
            __syncthreads();
            for (uint32_t b = tid; b < nb; b += WT_BT) {  // bucket b: [end of b - 1, end of b)
                const uint32_t lo = b ? bc[b - 1] : 0u, hi = bc[b];
                for (uint32_t i = lo + 1; i < hi; ++i) {
                    const uint64_t v = srt[i];
                    const uint16_t pv = posL[i];
                    uint32_t j = i;
                    while (j > lo && (srt[j - 1] > v || (srt[j - 1] == v && posL[j - 1] > pv))) {
                        srt[j] = srt[j - 1];
                        posL[j] = posL[j - 1];
                        --j;
                    }
                    srt[j] = v;
                    posL[j] = pv;
                }
            }
        } else {
#pragma unroll
            for (uint32_t k = 0; k < PPT; ++k) {
                const uint32_t i = tid + k * WT_BT;
                if (i < np) {
                    srt[i] = i < n ? h[k] : ~0ull;
                    posL[i] = (uint16_t)i;
                }
            }
            for (uint32_t k = 2; k <= np; k <<= 1)
                for (uint32_t j = k >> 1; j; j >>= 1) {
                    __syncthreads();
                    for (uint32_t i = tid; i < np; i += WT_BT) {
                        const uint32_t l = i ^ j;
                        if (l > i) {
                            const uint64_t a = srt[i], b = srt[l];
                            const uint16_t pa = posL[i], pb = posL[l];
                            if ((a > b || (a == b && pa > pb)) == ((i & k) == 0)) {
                                srt[i] = b;
                                srt[l] = a;
                                posL[i] = pb;
                                posL[l] = pa;
                            }
                        }
                    }
                }
        }
        __syncthreads();
        // the C-sorted entries (thread tid holds positions tid + k * WT_BT), written out as the table's row segment
        uint4 *__restrict__ out = hz.table + (uint64_t)L * E + ci.start;
#pragma unroll
        for (uint32_t k = 0; k < PPT; ++k) {
            const uint32_t j = tid + k * WT_BT;
            q[k] = make_uint4(0, 0, 0, 0);
            if (j < n) {
                const uint64_t C = srt[j];
                const uint32_t e = eL[posL[j]];
                q[k] = make_uint4((uint32_t)C, (uint32_t)(C >> 32), mod_barrett64(C, hz.m, hz.mu), ~e);
                out[j] = q[k];
            }
        }
        __syncthreads();  // posL (the key region) and srt are free again
    } else {
        const uint4 *__restrict__ row = table + (uint64_t)L * E + ci.start;
#pragma unroll
        for (uint32_t k = 0; k < PPT; ++k) {
            const uint32_t i = tid + k * WT_BT;
            q[k] = i < n ? row[i] : make_uint4(0, 0, 0, 0);
        }
    }
    uint64_t s = 0;
#pragma unroll
    for (uint32_t k = 0; k < PPT; ++k) s += q[k].z;
    for (int o = 32; o; o >>= 1) s += __shfl_xor(s, o, 64);
    if (lane == 0) part[wave] = s;
    __syncthreads();
    if (tid == 0) {
        unsigned long long t = 0;
        for (uint32_t w = 0; w < WT_BW; ++w) t += part[w];
        atomicAdd(rowsum + L, t);
    }
    WT_STAMP(1);
    if (n <= WT_BRUTE) return;
    uint32_t *chi_img = reinterpret_cast<uint32_t *>(img + ci.o_chi);
#pragma unroll
    for (uint32_t k = 0; k < PPT; ++k) {
        const uint32_t i = tid + k * WT_BT;
        if (i >= n) break;
        chi_img[i] = q[k].y;
        const uint32_t e = ~q[k].w;  // < 65536 (the host checks E)
        key[i] = ((uint64_t)q[k].z << 32) | ((uint64_t)(0xffffu - e) << 16) | i;
    }
    WT_STAMP(2);
    // sort the keys: counting sort on the top lg(np) - 1 bits of Cm (uniform in [0, m): ~2 keys per bucket), then an
    // insertion sort per bucket (a thread per bucket); a bucket of more than 32 keys (repeated hints: equal Cm)
    // sends the whole segment to a bitonic sort
    {
        const uint32_t sh = mbits > lgb ? mbits - lgb : 0u;
        for (uint32_t b = tid; b < nb; b += WT_BT) bc[b] = 0;
        __syncthreads();
        for (uint32_t i = tid; i < n; i += WT_BT) atomicAdd(&bc[(uint32_t)(key[i] >> 32) >> sh], 1u);
        __syncthreads();
        wt_bucket_scan(bc, nb, cum, bmax, tid);
        if (bmax[0] <= 32) {
            for (uint32_t i = tid; i < n; i += WT_BT) {
                const uint64_t kk = key[i];
                srt[atomicAdd(&bc[(uint32_t)(kk >> 32) >> sh], 1u)] = kk;
            }
            __syncthreads();
            for (uint32_t b = tid; b < nb; b += WT_BT) {  // bucket b: [end of b - 1, end of b)
                const uint32_t lo = b ? bc[b - 1] : 0u, hi = bc[b];
                for (uint32_t i = lo + 1; i < hi; ++i) {
                    const uint64_t v = srt[i];
                    uint32_t j = i;
                    while (j > lo && srt[j - 1] > v) {
                        srt[j] = srt[j - 1];
                        --j;
                    }
                    srt[j] = v;
                }
            }
        } else {
            for (uint32_t i = n + tid; i < np; i += WT_BT) key[i] = ~0ull;
            for (uint32_t k = 2; k <= np; k <<= 1)
                for (uint32_t j = k >> 1; j; j >>= 1) {
                    __syncthreads();
                    for (uint32_t i = tid; i < np; i += WT_BT) {
                        const uint32_t l = i ^ j;
                        if (l > i) {
                            const uint64_t a = key[i], b = key[l];
                            if ((a > b) == ((i & k) == 0)) {
                                key[i] = b;
                                key[l] = a;
                            }
                        }
                    }
                }
            __syncthreads();
            for (uint32_t i = tid; i < n; i += WT_BT) srt[i] = key[i];
        }
        __syncthreads();  // the keys' region becomes the rank arrays
        WT_STAMP(3);
    }
    uint32_t *chiL = reinterpret_cast<uint32_t *>(key) + WT_NMAX;  // C_hi by position (the bucket index below)
#pragma unroll
    for (uint32_t k = 0; k < PPT; ++k) {
        const uint32_t i = tid + k * WT_BT;
        if (i < n) chiL[i] = q[k].y;
    }
    uint32_t *cm_img = reinterpret_cast<uint32_t *>(img + ci.o_cm);
    uint16_t *e_img = reinterpret_cast<uint16_t *>(img + ci.o_e);
    for (uint32_t j = tid; j < n; j += WT_BT) {
        const uint64_t kk = srt[j];
        cm_img[j] = (uint32_t)(kk >> 32);
        e_img[j] = (uint16_t)(0xffffu - ((kk >> 16) & 0xffffu));
        S0[kk & 0xffffu] = (uint16_t)j;
    }
    if (tid < WT_PAD) {
        cm_img[n + tid] = ~0u;  // sentinels: never below a search bound
        chi_img[n + tid] = ~0u;
    }
    __syncthreads();  // chiL complete
    WT_STAMP(4);
    // bucket indexes (first rank with Cm >= b << msh, b <= 256; first position with C_hi >= b << 24, b < 256): every
    // position writes the buckets between its predecessor's and its own (the sorted order's boundaries)
    uint32_t *im = idx, *ic = idx + 260;
    for (uint32_t i = tid; i <= n; i += WT_BT) {
        const int bm = i < n ? (int)((uint32_t)(srt[i] >> 32) >> msh) : 257;
        const int pm_ = i ? (int)((uint32_t)(srt[i - 1] >> 32) >> msh) : -1;
        for (int b = pm_ + 1; b <= min(bm, 256); ++b) im[b] = i;
        const int bc2 = i < n ? (int)(chiL[i] >> 24) : 256;
        const int pc = i ? (int)(chiL[i - 1] >> 24) : -1;
        for (int b = pc + 1; b <= min(bc2, 255); ++b) ic[b] = i;
    }
    __syncthreads();
    if (tid < 257) {
        reinterpret_cast<uint16_t *>(img + ci.o_im)[tid] = (uint16_t)im[tid];
        atomicMax(bmax + 2, (tid < 256 ? im[tid + 1] : n) - im[tid]);
    }
    if (tid < 256) {
        reinterpret_cast<uint16_t *>(img + ci.o_ic)[tid] = (uint16_t)ic[tid];
        atomicMax(bmax + 3, (tid < 255 ? ic[tid + 1] : n) - ic[tid]);
    }
    __syncthreads();
    if (tid == 0) atomicMax(&classes[c].rS, 32u - __clz(max(bmax[2], bmax[3])));
    WT_STAMP(5);
    WT_STAMP(6);
    if constexpr (BB == 6) {
        if (ci.o_pl) {
            // rank-block planes instead of levels (wt_layout): plane b = [rank >= 64 b] in position order, b = 0 .. nbk
            // (plane 0 all ones, plane nbk all zeros: the sweep reads f_b(d) for every b it can form without a select),
            // one {32 bits, ones before} pair per 32 positions like a level. A wave takes every WT_BW-th plane and
            // walks the 64-position groups in order (ballot, running count); the same walk lists block b's ranks in
            // position order -- the node the level passes would have ended with -- for the block's prefix masks.
            const uint32_t nbk = (n >> 6) + 1, nw = ci.nw, ng = (nw + 1) / 2;
            uint2 *pl = reinterpret_cast<uint2 *>(img + ci.o_pl);
            uint64_t *mk = reinterpret_cast<uint64_t *>(img + ci.o_mk);
            uint8_t *ord = reinterpret_cast<uint8_t *>(bc) + 64 * wave;  // [64] the block's ranks mod 64 (bc is free)
            const uint64_t below = (1ull << lane) - 1ull;
            for (uint32_t b = wave; b <= nbk; b += WT_BW) {
                uint32_t pre = 0, inb = 0, wlo = 0, whi = 0, wpre = 0;  // lane g keeps group g's two words (ng <= 64)
#pragma unroll 4
                for (uint32_t g = 0; g < ng; ++g) {
                    const uint32_t j = g * 64 + lane, v = j < n ? S0[j] : 0u;
                    const uint64_t bg = __ballot(j < n && (v >> 6) >= b), be = __ballot(j < n && (v >> 6) == b);
                    if (lane == g) {
                        wlo = (uint32_t)bg;
                        whi = (uint32_t)(bg >> 32);
                        wpre = pre;
                    }
                    if (be >> lane & 1) ord[inb + (uint32_t)__popcll(be & below)] = (uint8_t)(v & 63);
                    pre += (uint32_t)__popcll(bg);
                    inb += (uint32_t)__popcll(be);
                }
                if (lane < ng) {
                    pl[b * nw + 2 * lane] = make_uint2(wlo, wpre);
                    if (2 * lane + 1 < nw) pl[b * nw + 2 * lane + 1] = make_uint2(whi, wpre + (uint32_t)__popc(wlo));
                }
                if (b < nbk) {  // entry o of block b = the OR of bit (rank mod 64) over the block's first o entries
                    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
                    __builtin_amdgcn_wave_barrier();
                    unsigned long long v = lane < inb ? 1ull << ord[lane] : 0ull;
                    for (int o = 1; o < 64; o <<= 1) {
                        const unsigned long long u = __shfl_up(v, o, 64);
                        if (lane >= (uint32_t)o) v |= u;
                    }
                    mk[b * 65 + lane + 1] = v;
                    if (lane == 0) mk[b * 65] = 0;
                    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
                    __builtin_amdgcn_wave_barrier();
                }
            }
            WT_STAMP(7);
#ifdef WT_BUILD_TRACE
            __syncthreads();
#endif
            WT_STAMP(8);
            return;
        }
    }
    // wavelet levels above the 32-rank blocks. Per level, wave w ballots a contiguous range of 64-position groups
    // (bit K-1-l of the rank at each position, in this level's order), the 8 wave totals give each wave its ones
    // before its range, and every position's destination in the next level's order follows from the ones before it
    // in its node: one barrier for the totals, one for the next order (no serial scan of the words).
    const uint32_t K = ci.K, nw = ci.nw, lb = wt_levels(K, BB);
    uint2 *lv = reinterpret_cast<uint2 *>(img + ci.o_lv);
    uint16_t *cur = S0, *nxt = S0 + WT_NMAX;
    constexpr uint32_t MAXG = (WT_NMAX / 64 + 1 + WT_BW - 1) / WT_BW;  // groups per wave, at most
    const uint32_t ng = (nw * 32 + 63) / 64, gpw = (ng + WT_BW - 1) / WT_BW, g0 = wave * gpw;
    uint32_t *wtot = cum;  // [WT_BW]
    for (uint32_t l = 0; l < lb; ++l) {
        const uint32_t h = 1u << (K - l - 1);
        uint64_t bal[MAXG];
        uint32_t vv[MAXG], tot = 0;
#pragma unroll
        for (uint32_t gi = 0; gi < MAXG; ++gi) {
            const uint32_t g = g0 + gi, j = g * 64 + lane;
            bal[gi] = 0;
            vv[gi] = 0;
            if (gi < gpw && g < ng) {
                vv[gi] = j < n ? cur[j] : 0u;
                bal[gi] = __ballot(j < n && (vv[gi] & h));
                tot += (uint32_t)__popcll(bal[gi]);
            }
        }
        if (lane == 0) wtot[wave] = tot;
        __syncthreads();
        uint32_t pre = 0;
        for (uint32_t w = 0; w < wave; ++w) pre += wtot[w];
        const uint64_t below = (1ull << lane) - 1ull;
#pragma unroll
        for (uint32_t gi = 0; gi < MAXG; ++gi) {
            const uint32_t g = g0 + gi, j = g * 64 + lane;
            if (gi < gpw && g < ng) {
                const uint64_t bg = bal[gi];
                if (lane == 0) lv[l * nw + 2 * g] = make_uint2((uint32_t)bg, pre);
                if (lane == 1 && 2 * g + 1 < nw)
                    lv[l * nw + 2 * g + 1] = make_uint2((uint32_t)(bg >> 32), pre + (uint32_t)__popc((uint32_t)bg));
                if (j < n) {
                    const uint32_t v = vv[gi];
                    const uint32_t s0 = v & ~(2 * h - 1);  // the node's first position
                    const uint32_t r1 = pre + (uint32_t)__popcll(bg & below) - (s0 >> 1);
                    nxt[(v & h) ? s0 + h + r1 : j - r1] = (uint16_t)v;
                }
                pre += (uint32_t)__popcll(bg);
            }
        }
        __syncthreads();
        uint16_t *t = cur;
        cur = nxt;
        nxt = t;
    }
    WT_STAMP(7);
    // level lb: the node of block b holds the ranks [2^BB b, 2^BB (b + 1)) in position order (all n ranks when K <= BB);
    // entry o of block b = the OR of bit (rank mod 2^BB) over the block's first o entries: a prefix OR per block
    const uint32_t nbk = (n >> BB) + 1;
    if constexpr (BB == 5) {  // two blocks per wave step, 32 lanes each
        uint32_t *mk = reinterpret_cast<uint32_t *>(img + ci.o_mk);
        for (uint32_t b0 = 2 * wave; b0 < nbk; b0 += 2 * WT_BW) {
            const uint32_t b = b0 + (lane >> 5), j = 32 * b + (lane & 31);
            uint32_t v = (b < nbk && j < n) ? 1u << (cur[j] & 31) : 0u;
            for (int o = 1; o < 32; o <<= 1) {
                const uint32_t u = __shfl_up(v, o, 64);
                if ((lane & 31) >= (uint32_t)o) v |= u;
            }
            if (b < nbk) {
                mk[b * 33 + (lane & 31) + 1] = v;
                if ((lane & 31) == 0) mk[b * 33] = 0;
            }
        }
    } else if constexpr (BB == 6) {  // a block per wave step
        uint64_t *mk = reinterpret_cast<uint64_t *>(img + ci.o_mk);
        for (uint32_t b = wave; b < nbk; b += WT_BW) {
            const uint32_t j = 64 * b + lane;
            unsigned long long v = j < n ? 1ull << (cur[j] & 63) : 0ull;
            for (int o = 1; o < 64; o <<= 1) {
                const unsigned long long u = __shfl_up(v, o, 64);
                if (lane >= (uint32_t)o) v |= u;
            }
            mk[b * 65 + lane + 1] = v;
            if (lane == 0) mk[b * 65] = 0;
        }
    } else {  // a block per wave step, in two halves of 64 entries (the second half ORs in the first's total)
        uint4 *mk = reinterpret_cast<uint4 *>(img + ci.o_mk);
        for (uint32_t b = wave; b < nbk; b += WT_BW) {
            unsigned long long clo = 0, chi = 0;
            for (uint32_t hf = 0; hf < 2; ++hf) {
                const uint32_t j = 128 * b + 64 * hf + lane, r = j < n ? (uint32_t)(cur[j] & 127) : 0u;
                unsigned long long lo = (j < n && r < 64) ? 1ull << r : 0ull;
                unsigned long long hi = (j < n && r >= 64) ? 1ull << (r - 64) : 0ull;
                for (int o = 1; o < 64; o <<= 1) {
                    const unsigned long long ul = __shfl_up(lo, o, 64), uh = __shfl_up(hi, o, 64);
                    if (lane >= (uint32_t)o) {
                        lo |= ul;
                        hi |= uh;
                    }
                }
                lo |= clo;
                hi |= chi;
                mk[b * 129 + 64 * hf + lane + 1] =
                    make_uint4((uint32_t)lo, (uint32_t)(lo >> 32), (uint32_t)hi, (uint32_t)(hi >> 32));
                clo = __shfl(lo, 63, 64);
                chi = __shfl(hi, 63, 64);
            }
            if (lane == 0) mk[b * 129] = make_uint4(0u, 0u, 0u, 0u);
        }
    }
#ifdef WT_BUILD_TRACE
    __syncthreads();
#endif
    WT_STAMP(8);
}

// ---------------------------------------------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------------------------------------------
static uint32_t bitlen(uint64_t x) {
    uint32_t b = 0;
    while (x) {
        ++b;
        x >>= 1;
    }
    return b;
}

// read at every plan build (tests switch it per plan)
bool wt_enabled() {
    const char *e = ab_env("NMZ_REPLAY_WT");
    return !(e && std::string(e) == "0");
}

// the widest rank blocks a plan may take: 64 ranks (NMZ_WT_BB = 5 | 6 | 7, A/B and tests; read at every plan build)
static uint32_t wt_max_bb() {
    const char *e = ab_env("NMZ_WT_BB");
    const int v = e ? atoi(e) : 6;
    return (uint32_t)((v >= 5 && v <= 7) ? v : 6);
}

// rank-block planes (bb = 6) in place of a plan's levels: NMZ_WT_PLANES=0 keeps the levels (A/B and tests; read at
// every plan build)
static bool wt_planes_enabled() {
    const char *e = ab_env("NMZ_WT_PLANES");
    return !(e && std::string(e) == "0");
}

// the plan kernel's forms: every launch and the LDS attribute take the kernel from here
using WtBuildKernel = decltype(&k_replayable_wt_build<false, 5>);
static WtBuildKernel wt_build_kernel(bool fused, uint32_t bb) {
    return fused ? (bb == 7   ? k_replayable_wt_build<true, 7>
                    : bb == 6 ? k_replayable_wt_build<true, 6>
                              : k_replayable_wt_build<true, 5>)
                 : (bb == 7   ? k_replayable_wt_build<false, 7>
                    : bb == 6 ? k_replayable_wt_build<false, 6>
                              : k_replayable_wt_build<false, 5>);
}
static bool wt_build_lds_attr() {
    for (bool fused : {false, true})
        for (uint32_t bb = 5; bb <= 7; ++bb)
            if (hipFuncSetAttribute(reinterpret_cast<const void *>(wt_build_kernel(fused, bb)),
                                    hipFuncAttributeMaxDynamicSharedMemorySize, (int)WT_LDS_MAX) != hipSuccess)
                return false;
    return true;
}

static uint64_t r16(uint64_t b) { return (b + 15) & ~15ull; }

// the segments' descriptors for rank blocks of 2^bb ranks, with planes or levels; returns the row image's bytes
static uint64_t wt_layout_image(std::vector<WtClass> &oc, const std::vector<ClassInfo> &seg, uint32_t bb, bool planes) {
    oc.assign(seg.size(), WtClass{});
    uint64_t off = 0;
    for (size_t c = 0; c < seg.size(); ++c) {
        WtClass &o = oc[c];
        o.pn = seg[c].pn;
        o.start = seg[c].start;
        o.n = seg[c].count;
        if (o.n <= WT_BRUTE) continue;
        o.K = bitlen(o.n);  // 2^K > n >= every bound R
        o.nw = o.n / 32 + 1;
        o.o_lv = (uint32_t)off;
        off += r16(planes ? 0 : (uint64_t)wt_levels(o.K, bb) * o.nw * 8);
        o.o_cm = (uint32_t)off;
        off += r16((uint64_t)(o.n + WT_PAD) * 4);
        o.o_chi = (uint32_t)off;
        off += r16((uint64_t)(o.n + WT_PAD) * 4);
        o.o_e = (uint32_t)off;
        off += r16((uint64_t)o.n * 2);
        o.o_im = (uint32_t)off;
        off += r16(257 * 2);
        o.o_ic = (uint32_t)off;
        off += r16(256 * 2);
        o.o_mk = (uint32_t)off;
        off += r16(wt_mask_bytes(o.n, bb));
        if (planes) {  // planes 0 .. (n >> 6) + 1 (never at offset 0: the segment's other arrays come first)
            o.o_pl = (uint32_t)off;
            off += r16(wt_plane_bytes(o.n, o.nw));
        }
    }
    return off;
}

bool wt_layout(WtState &w, nmz_ctx *ctx, uint32_t E, const ClassInfo *cls, uint32_t n_cls, const ModParams &mod,
               bool fused, std::vector<WtClass> &oc) {
    w.on = false;
    if (!wt_enabled() || !mod.m32ok || E == 0 || E > 65536) return false;
    if (fused) {  // every class is one segment the plan kernel sorts itself
        for (uint32_t c = 0; c < n_cls; ++c)
            if (cls[c].count > WT_NMAX - 1) return false;
    }
    // segments: a class of 4,096 events or more (the plan kernel sorts < 4,096 keys in LDS) splits into near-equal
    // C-sorted sub-segments, each one a segment in its own right (every decision of it is (base + Cm) mod m with
    // the same carry rule C > ~H, just over fewer events)
    std::vector<ClassInfo> seg;
    for (uint32_t c = 0; c < n_cls; ++c) {
        const uint32_t n = cls[c].count, parts = (n + WT_NMAX - 2) / (WT_NMAX - 1);
        for (uint32_t k = 0, lo = 0; k < parts; ++k) {
            const uint32_t len = n / parts + (k < n % parts ? 1u : 0u);
            seg.push_back(ClassInfo{cls[c].pn, cls[c].start + lo, len});
            lo += len;
        }
    }
    n_cls = (uint32_t)seg.size();
    // the widest rank blocks whose row image fits LDS (NMZ_WT_BB caps the width, A/B and tests)
    uint32_t bb = wt_max_bb();
    uint64_t off = wt_layout_image(oc, seg, bb, false);
    while (bb > 5 && std::max<uint64_t>(16, r16(off)) + 32 > WT_LDS_MAX) off = wt_layout_image(oc, seg, --bb, false);
    // 64-rank blocks: planes instead of levels while the image stays within WT_PLANES_MAX (NMZ_WT_PLANES=0: levels)
    bool planes = false;
    if (bb == 6 && wt_planes_enabled()) {
        const uint64_t poff = wt_layout_image(oc, seg, 6, true);
        planes = std::max<uint64_t>(16, r16(poff)) <= WT_PLANES_MAX;
        off = planes ? poff : wt_layout_image(oc, seg, 6, false);
    }
    {  // the plan kernel's dispatch order: segments by size, largest first
        std::vector<uint32_t> ord(n_cls);
        std::iota(ord.begin(), ord.end(), 0u);
        std::stable_sort(ord.begin(), ord.end(), [&](uint32_t a, uint32_t b) { return oc[a].n > oc[b].n; });
        for (uint32_t r = 0; r < n_cls; ++r) oc[r].order = ord[r];
    }
    const uint64_t rb = std::max<uint64_t>(16, r16(off));
    if (rb + 32 > WT_LDS_MAX) return false;
    // function attributes are per device: once per context (a context owns one device; its calls are serialised)
    if (!ctx->wt_lds_attr) {
        if (!wt_sweep_lds_attr() || !wt_build_lds_attr()) {
            (void)hipGetLastError();  // not sticky for the launches that follow: keep the order-query sweep
            return false;
        }
        ctx->wt_lds_attr = true;
    }
    w.rb16 = (uint32_t)(rb / 16);
    w.bb = bb;
    w.planes = planes;
    w.n_classes = n_cls;
    w.msh = mod.m32 > 255 ? bitlen(mod.m32) - 8 : 0;
    return true;
}

int wt_launch(WtState &w, const uint4 *d_table, uint32_t E, const ModParams &mod, hipStream_t st,
              const WtPlanHints *hints, WtClass *d_cls, unsigned long long *d_rowsum, bool sync) {
    ScratchLayout lay;
    NMZ_TRY(lay.add(&w.d_blob, 256 * (size_t)w.rb16).bind(w.mem));
    w.d_rowsum = d_rowsum;
    w.d_classes = d_cls;
    WtHints hz{};
    if (hints)
        hz = WtHints{hints->hoff, hints->hbytes, hints->perm, mod.m, mod.mu, hints->table, hints->zero0, hints->n_zero0,
                     hints->zero1, hints->n_zero1};
    hipLaunchKernelGGL(wt_build_kernel(hints != nullptr, w.bb), dim3(w.n_classes, 256), dim3(WT_BT), WtBuildLds::total,
                       st, hints ? nullptr : d_table, E, d_cls, w.msh, bitlen(mod.m32), w.d_blob, w.rb16, d_rowsum, hz);
    NMZ_HIP(hipGetLastError());
    if (sync) NMZ_HIP(hipStreamSynchronize(st));  // the plan is complete when it is returned
    w.on = true;
    return NMZ_OK;
}

int wt_build(WtState &w, nmz_ctx *ctx, const uint4 *d_table, uint32_t E, const ClassInfo *cls, uint32_t n_cls,
             const ModParams &mod, hipStream_t st) {
    std::vector<WtClass> oc;
    if (!wt_layout(w, ctx, E, cls, n_cls, mod, false, oc)) return NMZ_OK;
    // classes and row sums in their own buffer (the fused path uploads them with the plan's inputs)
    unsigned long long *d_rowsum;
    WtClass *d_cls;
    ScratchLayout lay;
    NMZ_TRY(lay.add(&d_rowsum, 256).add(&d_cls, oc.size()).bind(w.aux));
    NMZ_HIP(hipMemsetAsync(d_rowsum, 0, 256 * 8, st));
    NMZ_TRY(ctx->pin[1].ensure(oc.size() * sizeof(WtClass)));
    std::memcpy(ctx->pin[1].ptr, oc.data(), oc.size() * sizeof(WtClass));
    NMZ_HIP(hipMemcpyAsync(d_cls, ctx->pin[1].ptr, oc.size() * sizeof(WtClass), hipMemcpyHostToDevice, st));
    NMZ_TRY(ctx->pin[1].mark(st));
    return wt_launch(w, d_table, E, mod, st, nullptr, d_cls, d_rowsum, true);
}

}  // namespace nmz

#ifdef WT_BUILD_TRACE
extern "C" int nmz_debug_wt_build_trace(unsigned long long *out, uint32_t n) {
    const uint32_t m = std::min<uint32_t>(n, nmz::WT_TRACE_WGS * nmz::WT_TRACE_PHASES);
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(nmz::g_wt_build_trace), m * 8) == hipSuccess ? 0 : -1;
}
#endif
