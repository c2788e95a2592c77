// Top-k lists of the edit-distance kernels (ed.hip, ed_bv.hip, ed_wide.hip): k u64 slots per trace, ascending keys
// dist << 32 | id, UINT64_MAX = empty; cascade atomicMin insertion, lock-free and order-independent.
#pragma once
#include "nmz_common.h"

namespace nmz {

__device__ __forceinline__ void knn_insert(uint64_t *list, uint32_t k, uint64_t key) {
    if (key >= __hip_atomic_load(&list[k - 1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return;
    for (uint32_t s = 0; s < k; ++s) {
        const uint64_t old = atomicMin((unsigned long long *)&list[s], (unsigned long long)key);
        if (old == UINT64_MAX) return;
        key = old > key ? old : key;
    }
}

__device__ __forceinline__ uint64_t wave_min_u64(uint64_t v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const uint64_t o = __shfl_xor(v, off, 64);
        v = o < v ? o : v;
    }
    return v;
}

// insert the wave's k best keys for one query trace (all lanes participate)
__device__ __forceinline__ void knn_insert_wave(uint64_t *list, uint32_t k, uint64_t key, uint32_t lane) {
    for (uint32_t r = 0; r < k; ++r) {
        const uint64_t best = wave_min_u64(key);
        if (best == UINT64_MAX) return;
        if (best >= __hip_atomic_load(&list[k - 1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return;
        if (lane == (uint32_t)__builtin_amdgcn_readfirstlane(__ffsll(__ballot(key == best)) - 1))
            knn_insert(list, k, best);
        if (key == best) key = UINT64_MAX;
    }
}

}  // namespace nmz
