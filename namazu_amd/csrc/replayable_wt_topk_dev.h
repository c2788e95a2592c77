// K1 -- top-k on the wavelet-tree path (k <= 64; order: sum desc as int64, seed asc; n_fault = 0 for this policy).
// The sweep (replayable_wt.hip) leaves one record per chunk of 64 seeds: the chunk's largest sum (as an
// order-preserving key), the sorted position of its first seed and its seed count, at slot chunk_base[L] + ch
// (chunk_base[L] = the chunks of the rows before L, derived from bucket_off by the sweep and by the selection alike).
// Every slot of [0, n_chunks) is written exactly once per launch and none beyond is read: no init pass, no
// device-scope atomic, no fence. The chunks are disjoint groups of seeds, so the k-th largest chunk maximum tau is a
// value at least k seeds reach: no seed below it is in the top k, and only the seeds of the ~k chunks at or above tau
// need looking at. One one-block kernel (k_wt_topk_chunks) finds tau (a radix select over the chunk keys), reads those
// chunks' sums from the caller's stats, sorts the candidates (bitonic, LDS) and writes the k entries; more than
// WT_CAND flagged chunks or candidates (heavy ties, e.g. maxInterval 1) take a slow exact selection over the stats
// instead. The records and the candidate arrays are the scratch of replayable_wt_dev.h.
//
// Device code only, for replayable_wt.hip, which includes it after the sweep and launches the kernel (wt_topk). The
// kernel is compiled in the sweep's translation unit on purpose: in a module of its own the same source compiles to
// other machine code (the HIP headers' static helpers are then inlined in another order), 128 VGPRs and 36 bytes of
// scratch per lane instead of 127 and none.
#pragma once
#include "nmz_common.h"
#include "nmz_internal.h"
#include "replayable_plan.h"
#include "replayable_wt_dev.h"

namespace nmz {

__device__ __forceinline__ bool wt_better(unsigned long long ka, uint64_t sa, unsigned long long kb, uint64_t sb) {
    return ka > kb || (ka == kb && sa < sb);
}

// The selection, one workgroup: (a) n_chunks from bucket_off, as the sweep derives its slots; (b) tau = the k-th
// largest chunk key, by a radix select over 8-bit digits with an LDS histogram, starting below the highest bit in
// which any two keys differ (sums are non-negative and small: four digit passes at configs[1]), or 0 when there are
// fewer chunks than k; (c) the chunks at or above tau are listed in LDS and their seeds' sums read from the stats,
// the seeds at or above tau become the candidates (counter in LDS); (d) the candidates sorted and the k entries
// written; (e) more than WT_CAND flagged chunks or candidates: the exact selection one rank at a time over the stats
// in seed order.
// Chunk keys: the first WT_SEL_KPT per thread stay in registers over the digit passes (33 x 512 threads cover
// configs[1]'s ~16,600 chunks), the rest are read again; reading all of them again on every pass took the kernel
// alone from 36 to 60 us. One CU's memory throughput bounds the kernel (alone ~32 us: 266 KB of records, then
// ~6,000 scattered stats rows); beside the neighbouring steps' sweeps it costs the pipelined step ~1-2 us.
// Static LDS 26.7 KB (27,312 B: the sort's 25.5 KB -- the list of flagged chunks lies in the same arrays before the
// sort -- plus the 1 KB histogram and ~0.2 KB of scalars) and at most 128 VGPRs at 512 threads: the kernel fits beside
// a K1 workgroup with an 84 KB row image (when the select did not, it waited for a whole CU: +8 us per configs[1]
// step; 1,024 threads at 128 VGPRs do not fit either: step 56.0 -> 68.3 us).
#ifndef NMZ_WT_SEL_THREADS
#define NMZ_WT_SEL_THREADS 512
#endif
#ifndef NMZ_WT_SEL_KPT
#define NMZ_WT_SEL_KPT 33
#endif
constexpr uint32_t WT_SEL_THREADS = NMZ_WT_SEL_THREADS, WT_SEL_KPT = NMZ_WT_SEL_KPT;
constexpr uint32_t WT_SEL_CHUNK = 2048, WT_SEL_KEEP = (WT_CAND / WT_SEL_CHUNK) * 64;
template <uint32_t CS>
__global__ __launch_bounds__(WT_SEL_THREADS) __attribute__((amdgpu_waves_per_eu(4))) void k_wt_topk_chunks(const uint32_t *__restrict__ bucket_off,
                                                                   const WtChunkRec *__restrict__ rec,
                                                                   const uint32_t *__restrict__ sorted_idx,
                                                                   const nmz_sched_stats *__restrict__ stats,
                                                                   uint64_t S, uint64_t seed0, uint32_t k,
                                                                   uint32_t nmax, WtTopkState *__restrict__ tk,
                                                                   nmz_topk_entry *__restrict__ out) {
    constexpr uint32_t NT = WT_SEL_THREADS, NW = NT / 64, KPT = WT_SEL_KPT;
    static_assert(NT >= 256 && NT % 64 == 0 && CS <= 65535 && 2 * WT_SEL_CHUNK == WT_CAND, "selection layout");
    // candidates sorted in chunks of WT_SEL_CHUNK, each chunk's best k kept aside, then the kept ones sorted: 26 KB of
    // LDS instead of 48 for one sort of WT_CAND
    __shared__ unsigned long long ck[WT_SEL_CHUNK];
    __shared__ uint32_t ci[WT_SEL_CHUNK];
    __shared__ unsigned long long sk[WT_SEL_KEEP];
    __shared__ uint32_t si[WT_SEL_KEEP];
    __shared__ unsigned long long bk[NW], bs[NW];
    __shared__ uint32_t hist[256];
    __shared__ uint32_t wtot[NW], sel[2], cnt_s[2];  // cnt_s: flagged chunks, candidates
    uint32_t *fpos = reinterpret_cast<uint32_t *>(ck);  // [WT_CAND] the flagged chunks' first positions and seed
    uint16_t *fcnt = reinterpret_cast<uint16_t *>(ci);  // [WT_CAND] counts, until the sort takes the arrays
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const unsigned long long below = (1ull << lane) - 1ull;
    auto sentinel = [] {
        nmz_topk_entry e;
        e.seed = UINT64_MAX;
        e.sum_delay_ns = INT64_MIN;
        e.n_fault = 0;
        e.first_fault = NMZ_NONE;
        return e;
    };
    // few instructions on a long chain of loads and barriers, beside workgroups of the neighbouring steps' sweeps
    // that fill every issue slot: the chain's latency is what the step waits for
    __builtin_amdgcn_s_setprio(3);
    // the chunk keys, every load in flight together with the rows' offsets: loaded up to the records allocated
    // (nmax >= n_chunks; a slot past n_chunks holds nothing of this sweep and is masked below)
    unsigned long long kreg[KPT];
#pragma unroll
    for (uint32_t r = 0; r < KPT; ++r) {
        const uint32_t i = tid + r * NT;
        kreg[r] = i < nmax ? rec[i].key : 0ull;
    }
    const unsigned long long k0 = rec[0].key;
    // (a) the rows' chunks
    {
        uint32_t v = tid < 256 ? (bucket_off[tid + 1] - bucket_off[tid] + CS - 1) / CS : 0u;
        for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o, 64);
        if (lane == 0) wtot[wave] = v;
        if (tid < 2) cnt_s[tid] = 0;
    }
    __syncthreads();
    const uint32_t n = wtot[0] + wtot[1] + wtot[2] + wtot[3];
    // (b) tau. The keys agree above bit hb, the highest bit in which any of them differs from the first. The select
    // works on 32-bit keys, bits [sh0, sh0 + 32) of the chunk keys with sh0 = max(hb - 32, 0): all the bits that
    // differ when hb <= 32 (sums are small), and tau is then the exact k-th largest chunk key; a wider spread leaves
    // tau that key rounded down to a multiple of 2^sh0, still a value k chunk maxima reach. Half the registers and
    // half the instructions of 64-bit keys: the waves run their passes one dependent instruction after another
    const bool all = n < k;  // fewer chunks than k: tau 0, every seed a candidate
    unsigned long long tau = 0;
    uint32_t hb = 0;
    if (!all) {
        unsigned long long diff = 0;
#pragma unroll
        for (uint32_t r = 0; r < KPT; ++r) diff |= tid + r * NT < n ? kreg[r] ^ k0 : 0ull;
        for (uint32_t i = tid + KPT * NT; i < n; i += NT) diff |= rec[i].key ^ k0;
        for (int o = 32; o; o >>= 1) diff |= __shfl_xor(diff, o, 64);
        if (lane == 0) bk[wave] = diff;
        __syncthreads();
        diff = 0;
        for (uint32_t w = 0; w < NW; ++w) diff |= bk[w];
        hb = diff ? 64u - (uint32_t)__clzll(diff) : 0u;
    }
    const uint32_t sh0 = hb > 32 ? hb - 32 : 0;
    uint32_t w32[KPT], t32 = 0;
#pragma unroll
    for (uint32_t r = 0; r < KPT; ++r) w32[r] = (uint32_t)(kreg[r] >> sh0);
    if (!all) {
        // one digit per pass from the top: the digit's histogram over the keys that match the prefix so far, then the
        // bin holding the kk-th largest of them. A thread adds a run of equal digits with one atomic (the first
        // pass's keys crowd into a few bins)
        uint32_t sh = min(hb, 32u), kk = k;
        uint32_t pref = sh >= 32 ? 0u : ((uint32_t)(k0 >> sh0) >> sh) << sh;
        while (sh) {
            const uint32_t hi = sh, w = min(8u, sh);
            sh -= w;
            const uint32_t dm = (1u << w) - 1u;
            if (tid < 256) hist[tid] = 0;
            __syncthreads();
            uint32_t cur = 0, cnt = 0;
            auto add = [&](uint32_t key) {
                if (hi >= 32 || (key >> hi) == (pref >> hi)) {
                    const uint32_t d = (key >> sh) & dm;
                    if (d != cur && cnt) {
                        atomicAdd(&hist[cur], cnt);
                        cnt = 0;
                    }
                    cur = d;
                    ++cnt;
                }
            };
#pragma unroll
            for (uint32_t r = 0; r < KPT; ++r)
                if (tid + r * NT < n) add(w32[r]);
            for (uint32_t i = tid + KPT * NT; i < n; i += NT) add((uint32_t)(rec[i].key >> sh0));
            if (cnt) atomicAdd(&hist[cur], cnt);
            __syncthreads();
            // bins from the top: thread t holds bin 255 - t, an inclusive scan gives the keys at or above its bin
            uint32_t c = 0, inc = 0;
            if (tid < 256) {
                c = inc = hist[255 - tid];
                for (int o = 1; o < 64; o <<= 1) {
                    const uint32_t v = __shfl_up(inc, o, 64);
                    if (lane >= (uint32_t)o) inc += v;
                }
                if (lane == 63) wtot[wave] = inc;
            }
            __syncthreads();
            if (tid < 256) {
                for (uint32_t x = 0; x < wave; ++x) inc += wtot[x];
                if (inc - c < kk && kk <= inc) {  // one bin: at least kk keys match the prefix
                    sel[0] = 255 - tid;
                    sel[1] = kk - (inc - c);
                }
            }
            __syncthreads();
            pref |= sel[0] << sh;
            kk = sel[1];
        }
        t32 = pref;
        tau = (sh0 + 32 >= 64 ? 0ull : (k0 >> (sh0 + 32)) << (sh0 + 32)) | ((unsigned long long)pref << sh0);
    }
    // (c) the chunks at or above tau, listed in LDS: a thread marks its keys, then adds each marked one (~k in all)
    {
        static_assert(KPT <= 64, "one mark bit per register key");
        auto list = [&](uint32_t i) {
            const uint32_t slot = atomicAdd(&cnt_s[0], 1u);
            if (slot < WT_CAND) {
                fpos[slot] = rec[i].pos;
                fcnt[slot] = (uint16_t)rec[i].cnt;
            }
        };
        unsigned long long fm = 0;
#pragma unroll
        for (uint32_t r = 0; r < KPT; ++r) fm |= (tid + r * NT < n && (all || w32[r] >= t32)) ? 1ull << r : 0ull;
        while (fm) {
            const uint32_t r = (uint32_t)__ffsll((long long)fm) - 1u;
            fm &= fm - 1ull;
            list(tid + r * NT);
        }
        for (uint32_t i = tid + KPT * NT; i < n; i += NT)
            if (all || (uint32_t)(rec[i].key >> sh0) >= t32) list(i);
    }
    __syncthreads();
    const uint32_t nf = cnt_s[0];
    // an item per (flagged chunk, seed of it): U items per thread per round, their indices and then their sums in
    // flight together (two dependent round trips per round; ~k flagged chunks make one round). The candidates of a
    // single round stay in registers until the list of chunks is read, then go straight into the sort's arrays
    constexpr uint32_t U = 16;
    const uint32_t items = nf * CS;
    const bool one = nf <= WT_CAND && items <= U * NT;
    uint32_t idx[U], slot[U], fl = 0;
    unsigned long long key[U];
    if (nf <= WT_CAND) {
        for (uint32_t i0 = 0; i0 < items; i0 += U * NT) {
            bool ok[U];
            fl = 0;
#pragma unroll
            for (uint32_t u = 0; u < U; ++u) {
                const uint32_t it = i0 + u * NT + tid, fi = min(it / CS, nf - 1), o = it % CS;
                ok[u] = it < items && o < fcnt[fi];
                idx[u] = ok[u] ? sorted_idx[fpos[fi] + o] : 0u;
            }
#pragma unroll
            for (uint32_t u = 0; u < U; ++u) key[u] = ok[u] ? stats[idx[u]].sum_delay_ns ^ (1ull << 63) : 0ull;
#pragma unroll
            for (uint32_t u = 0; u < U; ++u) {
                const bool f = ok[u] && key[u] >= tau;
                const unsigned long long mask = __ballot(f);
                slot[u] = 0;
                if (mask) {
                    uint32_t base = 0;
                    if (lane == 0) base = atomicAdd(&cnt_s[1], (uint32_t)__popcll(mask));
                    base = __builtin_amdgcn_readfirstlane(base);
                    slot[u] = base + (uint32_t)__popcll(mask & below);
                    fl |= f ? 1u << u : 0u;
                    if (!one && f && slot[u] < WT_CAND) {
                        tk->cand_key[slot[u]] = key[u];
                        tk->cand_idx[slot[u]] = idx[u];
                    }
                }
            }
        }
        __syncthreads();  // the candidates counted (and, of several rounds, written), the list of chunks free
    }
    const uint32_t c = nf <= WT_CAND ? cnt_s[1] : WT_CAND + 1;
    const bool direct = one && c <= WT_SEL_CHUNK;  // one sort chunk, filled from the registers
    if (one && !direct && c <= WT_CAND) {
#pragma unroll
        for (uint32_t u = 0; u < U; ++u)
            if (fl >> u & 1u) {
                tk->cand_key[slot[u]] = key[u];
                tk->cand_idx[slot[u]] = idx[u];
            }
        __syncthreads();
    }
    if (c <= WT_CAND) {
        // (d) every seed at or above tau is a candidate: a bitonic sort of (key desc, seed asc) in LDS, padded with
        // key 0 (a real key has its top bit set: sums are non-negative)
        // bitonic sort of ck/ci[0, p2) (key desc, seed asc; padding last)
        auto sort = [&](uint32_t p2) {
            for (uint32_t kk = 2; kk <= p2; kk <<= 1)
                for (uint32_t j = kk >> 1; j; j >>= 1) {
                    __syncthreads();
                    for (uint32_t i = threadIdx.x; i < p2; i += NT) {
                        const uint32_t l = i ^ j;
                        if (l > i) {
                            const unsigned long long a = ck[i], b = ck[l];
                            const uint32_t ia = ci[i], ib = ci[l];
                            // l better than i
                            const bool lb = b > a || (b == a && b != 0 && seed0 + ib < seed0 + ia);
                            if (lb == ((i & kk) == 0)) {
                                ck[i] = b;
                                ck[l] = a;
                                ci[i] = ib;
                                ci[l] = ia;
                            }
                        }
                    }
                }
            __syncthreads();
        };
        auto pow2 = [](uint32_t x) {
            uint32_t p = 1;
            while (p < x) p <<= 1;
            return p;
        };
        const uint32_t nch = c > WT_SEL_CHUNK ? (c + WT_SEL_CHUNK - 1) / WT_SEL_CHUNK : 1;
        for (uint32_t q = 0; q < nch; ++q) {
            const uint32_t lo = q * WT_SEL_CHUNK, cc = min(c - lo, WT_SEL_CHUNK), p2 = pow2(cc);
            if (direct) {
                for (uint32_t i = cc + threadIdx.x; i < p2; i += NT) {
                    ck[i] = 0ull;
                    ci[i] = ~0u;
                }
#pragma unroll
                for (uint32_t u = 0; u < U; ++u)
                    if (fl >> u & 1u) {
                        ck[slot[u]] = key[u];
                        ci[slot[u]] = idx[u];
                    }
            } else {
                for (uint32_t i = threadIdx.x; i < p2; i += NT) {
                    ck[i] = i < cc ? tk->cand_key[lo + i] : 0ull;
                    ci[i] = i < cc ? tk->cand_idx[lo + i] : ~0u;
                }
            }
            sort(p2);
            if (nch > 1) {  // the chunk's best k aside (a seed outside them is beaten by k of this chunk alone)
                for (uint32_t i = threadIdx.x; i < k; i += NT) {
                    sk[q * k + i] = ck[i];
                    si[q * k + i] = ci[i];
                }
                __syncthreads();
            }
        }
        if (nch > 1) {
            const uint32_t p2 = pow2(nch * k);
            for (uint32_t i = threadIdx.x; i < p2; i += NT) {
                ck[i] = i < nch * k ? sk[i] : 0ull;
                ci[i] = i < nch * k ? si[i] : ~0u;
            }
            sort(p2);
        }
        for (uint32_t r = threadIdx.x; r < k; r += NT) {
            if (r < c) {
                nmz_topk_entry e;
                e.seed = seed0 + ci[r];  // seeds wrap as elsewhere
                e.sum_delay_ns = (int64_t)(ck[r] ^ (1ull << 63));
                e.n_fault = 0;
                e.first_fault = NMZ_NONE;
                out[r] = e;
            } else {
                out[r] = sentinel();  // fewer seeds than k
            }
        }
    } else {
        // (e) exact selection one rank at a time over the stats in seed order: the best entry after the previous one
        // in (key desc, seed asc)
        unsigned long long pk = ~0ull, ps = 0;
        bool first_rank = true;
        for (uint32_t r = 0; r < k; ++r) {
            unsigned long long mk = 0, ms = ~0ull;
            bool any = false;
            for (uint64_t i = threadIdx.x; i < S; i += NT) {
                const unsigned long long key = stats[i].sum_delay_ns ^ (1ull << 63), sd = seed0 + i;
                const bool after = first_rank || wt_better(pk, ps, key, sd);
                if (after && (!any || wt_better(key, sd, mk, ms))) {
                    mk = key;
                    ms = sd;
                    any = true;
                }
            }
            if (!any) mk = 0, ms = ~0ull;
            for (int o = 32; o; o >>= 1) {
                const unsigned long long ok = __shfl_xor(mk, o, 64), os = __shfl_xor(ms, o, 64);
                const bool oany = __shfl_xor((int)any, o, 64);
                if (oany && (!any || wt_better(ok, os, mk, ms))) {
                    mk = ok;
                    ms = os;
                    any = true;
                }
            }
            __syncthreads();
            if (lane == 0) {
                bk[threadIdx.x >> 6] = any ? mk : 0;
                bs[threadIdx.x >> 6] = any ? ms : ~0ull;
            }
            __syncthreads();
            // the block's best (empty slots hold key 0, seed ~0: never better than a real entry of key 0 with a
            // smaller seed; a real entry of key 0 and seed ~0 is found by the any flags below)
            unsigned long long bestk = 0, bests = ~0ull;
            bool found = false;
            for (uint32_t w = 0; w < NW; ++w) {
                const bool real = !(bk[w] == 0 && bs[w] == ~0ull);
                if (real && (!found || wt_better(bk[w], bs[w], bestk, bests))) {
                    bestk = bk[w];
                    bests = bs[w];
                    found = true;
                }
            }
            if (!found) {
                for (uint32_t q = r + threadIdx.x; q < k; q += NT) out[q] = sentinel();
                break;
            }
            if (threadIdx.x == 0) {
                nmz_topk_entry e;
                e.seed = bests;
                e.sum_delay_ns = (int64_t)(bestk ^ (1ull << 63));
                e.n_fault = 0;
                e.first_fault = NMZ_NONE;
                out[r] = e;
            }
            pk = bestk;
            ps = bests;
            first_rank = false;
        }
    }
}

}  // namespace nmz
