// Pieces of the random policy shared by its two translation units: K2 (random.hip, the delay + fault sweep) and
// the ProcSetEvent decisions (procset.hip). Go's generator by closed form for a run-time output index, the
// interval parameters, the seed decomposition of the sweeps, and the plan that holds the per-event FNV table.
#pragma once
#include "go_rand.h"
#include "nmz_common.h"

namespace nmz {

constexpr uint64_t MASK63 = 0x7fffffffffffffffULL;

// The device copy of rngCooked has external linkage (a static __constant__ is reached through the GOT, which changes
// K2's machine code), so each translation unit that includes this header names its own copy: NMZ_COOKED_TABLE,
// d_cooked unless the unit defines another name first.
#ifndef NMZ_COOKED_TABLE
#define NMZ_COOKED_TABLE d_cooked
#endif
__constant__ uint64_t NMZ_COOKED_TABLE[gorand::LEN] = NMZ_GO_RNG_COOKED_INIT;
[[maybe_unused]] __device__ const gorand::PowTable d_powa = gorand::make_pow_table();
// the same tables for the host decision paths (nmz_random_decide_host, nmz_procset_decide_host): the decision
// code is shared
[[maybe_unused]] static constexpr gorand::PowTable h_powa = gorand::make_pow_table();
[[maybe_unused]] static constexpr uint64_t h_cooked[gorand::LEN] = NMZ_GO_RNG_COOKED_INIT;
#ifdef __HIP_DEVICE_COMPILE__
#define NMZ_POWA(i) d_powa.v[i]
#define NMZ_COOKED(i) NMZ_COOKED_TABLE[i]
#else
#define NMZ_POWA(i) h_powa.v[i]
#define NMZ_COOKED(i) h_cooked[i]
#endif

// seeded vec[p] for a runtime index (slow path)
__host__ __device__ inline uint64_t vec_rt(uint32_t s, int p) {
    const uint32_t xa = gorand::modmul(s, NMZ_POWA(21 + 3 * p));
    const uint32_t xb = gorand::modmul(s, NMZ_POWA(22 + 3 * p));
    const uint32_t xc = gorand::modmul(s, NMZ_POWA(23 + 3 * p));
    const uint64_t ck = NMZ_COOKED(p);
    const uint32_t lo = (xb << 20) ^ xc ^ (uint32_t)ck;
    const uint32_t hi = (xa << 8) ^ (xb >> 12) ^ (uint32_t)(ck >> 32);
    return ((uint64_t)hi << 32) | lo;
}

// y_t for 0 <= t < 607: y_t = y_{t-607} + y_{t-273}, y_s (s<0) = vec[(333-s) mod 607]
__host__ __device__ inline uint64_t go_output(uint32_t s, int t) {
    uint64_t acc = 0;
    int u = t;
    while (u >= 0) {
        acc += vec_rt(s, (333 - (u - 607)) % 607);
        u -= 273;
    }
    return acc + vec_rt(s, ((333 - u) % 607 + 607) % 607);
}

struct ClassParams {
    int64_t min;
    uint64_t n;          // max - min (0 => fixed duration, no draw)
    uint64_t max_accept; // Int63n rejection bound
    uint64_t mu;         // floor(2^64 / n) (Barrett), 0 if n is a power of two
};

struct RandomKParams {
    ClassParams cls[2];
    int32_t fault_threshold;
};

// v mod n for v < 2^63, n not a power of two, mu = floor(2^64/n)
__host__ __device__ __forceinline__ uint64_t mod_barrett(uint64_t v, uint64_t n, uint64_t mu) {
    const uint64_t q = umulhi64(v, mu);
    uint64_t r = v - q * n;
    return r >= n ? r - n : r;
}

__device__ __forceinline__ uint4 uniform4(uint4 v) {
    return make_uint4(__builtin_amdgcn_readfirstlane(v.x), __builtin_amdgcn_readfirstlane(v.y),
                      __builtin_amdgcn_readfirstlane(v.z), __builtin_amdgcn_readfirstlane(v.w));
}

// Go seed for (prefix state h0 -> H = h0 * P^8, its residue Hm = H mod M31) and
// one table entry q = {C lo, C hi, C mod M31, class}
// nm = -M31 and one = 1 arrive in VGPRs the compiler cannot see through, so that both conditional corrections are
// a VOP2 borrow (v_sub_co) plus a VCC v_cndmask with VGPR operands (full rate) rather than an add of a literal and
// a v_min_u32 (half rate), and the s == 0 test is a borrow out of s - 1 rather than a v_cmp.
// Each correction fires about once in 2^31 decisions; the searched vectors of tests/golden/go_seed_edges.json
// (tools/find_go_seed_edges.c) take them, by class: the fold at s1 == M31 exactly and next to it (k0_s1_m31m1,
// k0_s1_m31, k0_s1_m31p1, k1_s1_m31, k2_s1_m31); the 4k borrow (k1_s1_m31, k1_t3, k2_s1_m31, k2_t7; wrap only and
// sign only for k = 1; t classes folded and, for a seed with Hm = 0, unfolded); the zero map (k0_s1_m31, k1_t4,
// k2_t8); s = 1 and s = M31 - 1 going into modmul / modmul_shl8 (k0_s1_m31p1, k1_t5, k2_t9; k0_s1_m31m1, k1_t3,
// k2_t7). tests/test_go_seed_edges_gpu.py runs them: test_random_sweep_on_the_vectors (both k_random_sweep
// instantiations, nm and one in VGPRs) and test_procset_on_the_vectors (k_procset_sweep, the default arguments).
__device__ __forceinline__ uint32_t go_seed_from_table(uint64_t H, uint32_t Hm, uint4 q,
                                                       uint32_t nm = gorand::NEG_M31, uint32_t one = 1u) {
    const uint64_t C = ((uint64_t)q.y << 32) | q.x;
    const uint64_t u = H + C;
    const uint32_t k = (uint32_t)(u < H) + (uint32_t)(u >> 63);  // wrap carry + sign
    uint32_t s1 = Hm + q.z, t;                                   // < 2*M31
    s1 = __builtin_sub_overflow(s1, 0u - nm, &t) ? s1 : t;
    uint32_t dd;
    const uint32_t s = __builtin_sub_overflow(s1, 4u * k, &dd) ? dd - nm : dd;
    return __builtin_sub_overflow(s, one, &t) ? 89482311u : s;
}

__host__ __device__ __forceinline__ uint64_t seed_prefix(uint64_t seed) {
    uint64_t h = FNV_OFFSET;
#pragma unroll
    for (int i = 0; i < 8; ++i) h = fnv_step(h, (uint32_t)(seed >> (8 * i)) & 0xff);
    return h;
}

}  // namespace nmz

struct nmz_random_plan {
    nmz_ctx *ctx = nullptr;
    uint32_t n_events = 0;
    nmz::RandomKParams kp{};
    uint4 *d_table = nullptr;
    uint64_t max_seeds = 0;
    nmz::DevBuf table_mem;
    nmz::DevBuf seed_scratch;
    nmz::DevBuf partial;  // per-chunk partial stats per seed slot (n_chunks > 1)
};

namespace nmz {

// random.hip: the resolved intervals in the kernels' form; a plan (per-event FNV table for evhash, class bits in
// the entries' w) with seed scratch for max_seeds seeds; its release; and the seeds seed0 .. seed0 + S - 1 hashed
// and bucketed by the low byte of their FNV prefix into work units of <= 64 seeds (*counter: a zeroed work-item
// counter)
int make_kparams(const nmz_random_params *p, RandomKParams &kp);
int random_plan_create(nmz_ctx *ctx, const uint64_t *evhash, const uint8_t *evclass, uint32_t E,
                       const nmz_random_params *params, uint64_t max_seeds, nmz_random_plan **out);
void random_plan_free(nmz_random_plan *p);
int random_bucket(nmz_random_plan *p, hipStream_t st, uint64_t seed0, uint64_t S, Buckets &b, uint32_t **counter);

}  // namespace nmz
