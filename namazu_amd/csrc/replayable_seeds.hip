// K1 -- seed prefixes: h0 = FNV-1a 64 of every seed string, with the bucket histogram of its low byte (the table
// row the seed reads), and the prepared seed sets built from them (nmz_replayable_seeds). order.hip borrows the
// kernels through seed_prefix_launch.
#include "nmz_common.h"
#include "nmz_internal.h"
#include "replayable_plan.h"

namespace nmz {

// ---------------------------------------------------------------------------
// seed prefix: h0 = FNV(seed bytes)
// ---------------------------------------------------------------------------
// A block's ppt * 256 seeds are contiguous in the CSR: their offsets and (when they fit SEED_LDS_BYTES) their bytes
// are staged in LDS with coalesced loads, and each thread hashes its seeds from LDS. (Per-thread global loads of a
// seed's offsets and bytes made every seed a chain of dependent global loads: ~21 us per 2^20 seeds.)
constexpr uint32_t SEED_LDS_BYTES = 16384;
constexpr uint32_t SEED_LDS_MAX_SEEDS = 256 * 16;
__global__ __launch_bounds__(256) void k_seed_prefix(const uint32_t *__restrict__ soff,
                                                     const uint8_t *__restrict__ sbytes, uint64_t n,
                                                     uint64_t *__restrict__ h0, uint32_t *__restrict__ rows) {
    // fused bucket histogram (low byte of h0): LDS counts, stored as the block's row of `rows` (Buckets)
    constexpr uint32_t ppt = BUCKET_PT;
    __shared__ uint32_t hist[256];
    __shared__ uint32_t so[SEED_LDS_MAX_SEEDS + 1];
    __shared__ uint32_t sb[SEED_LDS_BYTES / 4];
    hist[threadIdx.x] = 0;
    const uint64_t b0 = (uint64_t)blockIdx.x * 256 * ppt;
    const uint32_t nb = (uint32_t)min<uint64_t>(256 * (uint64_t)ppt, n - b0);
    const bool staged_off = nb <= SEED_LDS_MAX_SEEDS;
    if (staged_off)
        for (uint32_t i = threadIdx.x; i <= nb; i += 256) so[i] = soff[b0 + i];
    __syncthreads();
    const uint32_t B0 = staged_off ? so[0] : 0u, B1 = staged_off ? so[nb] : 0u;
    // LDS byte off0 + p holds seed byte B0 + p, off0 = the address's offset in its dword, so the whole dwords
    // between the first and last partial dword copy as aligned dwords (no byte outside [B0, B1) is read)
    const uint32_t off0 = (uint32_t)(reinterpret_cast<uintptr_t>(sbytes + B0) & 3u), total = B1 - B0;
    const bool staged = staged_off && off0 + total <= SEED_LDS_BYTES;
    const uint32_t A0 = B0 - off0;  // seed byte positions map to LDS byte (position - A0)
    if (staged) {
        uint8_t *lbw = reinterpret_cast<uint8_t *>(sb);
        const uint32_t head = min((4u - off0) & 3u, total), nint = (total - head) / 4, tail0 = head + 4 * nint;
        if (threadIdx.x < head) lbw[off0 + threadIdx.x] = sbytes[B0 + threadIdx.x];
        const uint32_t *src = reinterpret_cast<const uint32_t *>(sbytes + B0 + head);
        for (uint32_t i = threadIdx.x; i < nint; i += 256) sb[(off0 + head) / 4 + i] = src[i];
        if (threadIdx.x < total - tail0) lbw[off0 + tail0 + threadIdx.x] = sbytes[B0 + tail0 + threadIdx.x];
    }
    __syncthreads();
    const uint8_t *lb = reinterpret_cast<const uint8_t *>(sb);
    for (uint32_t r = 0; r < ppt; ++r) {
        const uint32_t i = r * 256 + threadIdx.x;
        if (i < nb) {
            uint64_t h = FNV_OFFSET;
            if (staged) {
                const uint32_t e = so[i + 1] - A0;
                for (uint32_t t = so[i] - A0; t < e; ++t) h = fnv_step(h, lb[t]);
            } else {
                uint32_t t = soff[b0 + i];
                const uint32_t end = soff[b0 + i + 1];
                // bytes up to a 4-byte boundary, then whole dwords, then the tail
                for (; t < end && (reinterpret_cast<uintptr_t>(sbytes + t) & 3); ++t) h = fnv_step(h, sbytes[t]);
                for (; t + 4 <= end; t += 4) {
                    const uint32_t w = *reinterpret_cast<const uint32_t *>(sbytes + t);
                    h = fnv_step(fnv_step(fnv_step(fnv_step(h, w & 0xff), (w >> 8) & 0xff), (w >> 16) & 0xff), w >> 24);
                }
                for (; t < end; ++t) h = fnv_step(h, sbytes[t]);
            }
            h0[b0 + i] = h;
            atomicAdd(&hist[h & 0xff], 1u);
        }
    }
    __syncthreads();
    rows[(size_t)blockIdx.x * 256 + threadIdx.x] = hist[threadIdx.x];
}

// FNV over the 9 decimal digits of x (< 10^9), most significant first; leading zeros are hashed only once
// `started` (a digit of a more significant part was nonzero)
__device__ __forceinline__ uint64_t fnv_dec9(uint64_t h, uint32_t x, bool &started) {
    constexpr uint32_t P10[9] = {1u, 10u, 100u, 1000u, 10000u, 100000u, 1000000u, 10000000u, 100000000u};
#pragma unroll
    for (int i = 8; i >= 0; --i) {
        const uint32_t d = x / P10[i];  // constant divisor: multiply-high + shift
        x -= d * P10[i];
        started |= d != 0;
        if (started) h = fnv_step(h, '0' + d);
    }
    return h;
}

// FNV(decimal string of v) from state h: strconv.FormatUint(v, 10) bytes
__device__ __forceinline__ uint64_t fnv_decimal_u64(uint64_t h, uint64_t v) {
    const uint64_t e18 = 1000000000000000000ull;
    const uint32_t c2 = (uint32_t)(v / e18);
    const uint64_t r = v - (uint64_t)c2 * e18;
    const uint32_t c1 = (uint32_t)(r / 1000000000ull), c0 = (uint32_t)(r - (uint64_t)c1 * 1000000000ull);
    bool started = false;
    h = fnv_dec9(h, c2, started);
    h = fnv_dec9(h, c1, started);
    h = fnv_dec9(h, c0, started);
    return started ? h : fnv_step(h, '0');
}

// seed prefix of the seeds "seed_lo" .. "seed_lo + n - 1" (decimal strings generated here: no seed CSR), with
// the same fused bucket histogram as k_seed_prefix. decimal(v) = decimal(v / 100) || two digits of v % 100 for
// v >= 100, and a block's 256 ppt consecutive seeds share at most 256 ppt / 100 + 2 prefixes v / 100: one lane per
// prefix hashes it (fnv_decimal_u64, ~300 VALU) into LDS once, then each seed takes its prefix's state and two FNV
// steps (~25 VALU per seed instead of ~300). Seeds below 100, and a block whose range wraps past 2^64, hash
// every seed in full.
constexpr uint32_t DEC_MAX_PREFIX = 64;  // 256 ppt / 100 + 2 <= 64 for ppt = BUCKET_PT <= 16
__global__ __launch_bounds__(256) void k_seed_prefix_decimal(uint64_t seed_lo, uint64_t n, uint64_t *__restrict__ h0,
                                                             uint32_t *__restrict__ rows) {
    constexpr uint32_t ppt = BUCKET_PT;
    __shared__ uint32_t hist[256];
    __shared__ uint64_t ph[DEC_MAX_PREFIX];
    hist[threadIdx.x] = 0;
    const uint64_t b0 = (uint64_t)blockIdx.x * 256 * ppt;
    const uint64_t nb = min<uint64_t>(256 * (uint64_t)ppt, n - b0);  // seeds of this block (>= 1)
    const uint64_t v0 = seed_lo + b0;
    const uint64_t P0 = v0 / 100;
    const uint32_t r0 = (uint32_t)(v0 - P0 * 100);
    const uint32_t np = (r0 + (uint32_t)nb - 1) / 100 + 1;  // prefixes P0 .. P0 + np - 1
    // the shared-prefix form: every seed >= 100, no wrap past 2^64, the prefixes fit the table
    const bool fast = v0 >= 100 && v0 + (nb - 1) >= v0 && np <= DEC_MAX_PREFIX;
    if (fast && threadIdx.x < np) ph[threadIdx.x] = fnv_decimal_u64(FNV_OFFSET, P0 + threadIdx.x);
    __syncthreads();
    for (uint32_t r = 0; r < ppt; ++r) {
        const uint32_t i = r * 256 + threadIdx.x;
        if (i < nb) {
            uint64_t h;
            if (fast) {
                const uint32_t x = r0 + i, q = x / 100, lo = x - q * 100, d1 = lo / 10;
                h = fnv_step(fnv_step(ph[q], '0' + d1), '0' + (lo - d1 * 10));
            } else {
                h = fnv_decimal_u64(FNV_OFFSET, v0 + i);
            }
            h0[b0 + i] = h;
            atomicAdd(&hist[h & 0xff], 1u);
        }
    }
    __syncthreads();
    rows[(size_t)blockIdx.x * 256 + threadIdx.x] = hist[threadIdx.x];
}

int seed_prefix_launch(hipStream_t st, const uint32_t *d_soff, const uint8_t *d_sbytes, uint64_t dec_lo, uint64_t S,
                       uint64_t *h0, uint32_t *rows) {
    if (S == 0) return NMZ_OK;
    if (d_soff)
        hipLaunchKernelGGL(k_seed_prefix, dim3(ceil_div(S, BUCKET_BLK)), dim3(256), 0, st, d_soff, d_sbytes, S, h0,
                           rows);
    else
        hipLaunchKernelGGL(k_seed_prefix_decimal, dim3(ceil_div(S, BUCKET_BLK)), dim3(256), 0, st, dec_lo, S, h0,
                           rows);
    NMZ_HIP(hipGetLastError());
    return NMZ_OK;
}

int seeds_create_locked(nmz_ctx *ctx, const uint32_t *d_seed_off, const uint8_t *d_seed_bytes, uint64_t n_seeds,
                        uint64_t dec_lo, nmz_replayable_seeds **out) {
    *out = nullptr;
    auto *s = new nmz_replayable_seeds();
    s->ctx = ctx;
    s->S = n_seeds;
    s->mem.pool = &ctx->pool;  // a stream of seed sets of one size reuses one buffer (no hipMalloc per set)
    hipStream_t st = ctx->stream;
    ScratchLayout lay;  // a seed scratch, then the copy of its row counts
    seed_scratch_layout(lay, n_seeds, s->sc);
    const int rc = lay.add(&s->hist, bucket_hist_u32(n_seeds)).bind(s->mem);
    if (rc != NMZ_OK) {
        delete s;
        return rc;
    }
    buckets_small(s->sc.small, s->sc.b);
    if (hipMemsetAsync(s->sc.counter, 0, 4 * sizeof(uint32_t), st) != hipSuccess ||
        seed_prefix_launch(st, d_seed_off, d_seed_bytes, dec_lo, n_seeds, s->sc.h0, s->sc.b.hist) != NMZ_OK ||
        hipMemcpyAsync(s->hist, s->sc.b.hist, bucket_hist_u32(n_seeds) * sizeof(uint32_t), hipMemcpyDeviceToDevice,
                       st) != hipSuccess ||
        bucket_seeds_counted(st, s->sc.h0, n_seeds, OQ_WG, s->sc.b, s->sc.counter) != NMZ_OK ||
        hipStreamSynchronize(st) != hipSuccess) {
        (void)hipStreamSynchronize(st);
        s->mem.release();
        delete s;
        return fail(NMZ_EHIP, "seed set build failed");
    }
    *out = s;
    return NMZ_OK;
}

void seeds_destroy_locked(nmz_replayable_seeds *seeds) {
    (void)hipDeviceSynchronize();  // sweeps on any stream may still read the set (its buffer goes to the pool)
    seeds->mem.release();
    delete seeds;
}

}  // namespace nmz

using namespace nmz;

extern "C" {

int nmz_replayable_seeds_create(nmz_ctx *ctx, const uint32_t *d_seed_off, const uint8_t *d_seed_bytes, uint64_t n_seeds,
                                uint64_t dec_lo, nmz_replayable_seeds **out) {
    NMZ_CHECK(ctx != nullptr && out != nullptr, "NULL argument");
    NMZ_CHECK(n_seeds >= 1 && n_seeds < (1ULL << 32), "1 <= n_seeds < 2^32");
    NMZ_CHECK(!d_seed_off || d_seed_bytes, "d_seed_bytes is NULL");
    CtxGuard g(ctx);
    NMZ_TRY(g.rc);
    return seeds_create_locked(ctx, d_seed_off, d_seed_bytes, n_seeds, dec_lo, out);
}

int nmz_replayable_seeds_destroy(nmz_replayable_seeds *seeds) {
    if (!seeds) return NMZ_OK;
    {
        CtxGuard g(seeds->ctx);
        seeds_destroy_locked(seeds);
    }
    return NMZ_OK;
}

}  // extern "C"
