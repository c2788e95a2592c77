// The trace signature's mix functions (unique.hip k_trace_sig, delivery.hip k_delivery_sweep and the host entry
// point nmz_replayable_delivery_host): a trace is the multiset {(symbol, rank)}, hashed by summing two 64-bit mixes
// of each pair mod 2^64, plus the element count (unique.hip's header comment has the argument).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace nmz {

__host__ __device__ __forceinline__ uint64_t fmix64(uint64_t x) {
    x ^= x >> 33;
    x *= 0xff51afd7ed558ccdULL;
    x ^= x >> 33;
    x *= 0xc4ceb9fe1a85ec53ULL;
    x ^= x >> 33;
    return x;
}

// per-rank keys: RANK_KEYS ranks in a table (computed once per context), larger ranks inline
constexpr uint32_t RANK_KEYS = 65536;

__host__ __device__ __forceinline__ uint64_t rank_key_a(uint32_t r) {
    return fmix64((uint64_t)r + 0x9e3779b97f4a7c15ULL);
}
__host__ __device__ __forceinline__ uint64_t rank_key_b(uint32_t r) {
    return fmix64(((uint64_t)r << 32 | (r ^ 0x5bd1e995u)) + 0x632be59bd9b4e019ULL);
}

// the pair (symbol s, rank r) -> two 64-bit summands: t = fmix64(s ^ ka(r)) and a second, different nonlinear
// function of t and kb(r) (one more 64-bit multiply instead of another fmix64)
__host__ __device__ __forceinline__ void mix2k(uint64_t s, ulonglong2 k, uint64_t &a, uint64_t &b) {
    const uint64_t t = fmix64(s ^ k.x);
    a = t;
    const uint64_t u = (t ^ k.y) * 0x94d049bb133111ebULL;
    b = u ^ (u >> 29);
}

// the signature's two words from the sums over the counted elements and their number
__host__ __device__ __forceinline__ uint64_t sig_final_lo(uint64_t acc1, uint32_t counted) {
    return acc1 + fmix64((uint64_t)counted + 1);
}
__host__ __device__ __forceinline__ uint64_t sig_final_hi(uint64_t acc2, uint32_t counted) {
    return acc2 ^ fmix64(((uint64_t)counted << 1) | 1);
}

}  // namespace nmz
