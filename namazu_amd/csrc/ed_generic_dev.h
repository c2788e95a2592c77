// The generic banded DP of k_ed_generic (ed.hip) and k_ed_query_generic (ed_query.hip).
#pragma once
#include "nmz_common.h"

namespace nmz {

// ED_W(a, b) with the band row D[t] = cell (i, i + t - W) in global scratch (column t at scratch[t * stride]):
// one thread per pair, any band, any symbol type
template <typename T>
__device__ uint32_t generic_band_dist(const T *__restrict__ a, int64_t n, const T *__restrict__ b, int64_t m, uint32_t W,
                                      uint32_t *__restrict__ scratch, uint64_t stride) {
    const uint32_t NB = 2 * W + 1;
    const uint32_t INF = 0x3fffffffu;
    const int64_t dd = m - n;
    if (dd > (int64_t)W || dd < -(int64_t)W) return W + 1;
    // row 0: D(0, j) = j
    for (uint32_t t = 0; t < NB; ++t) scratch[t * stride] = (t >= W) ? (t - W) : INF;
    for (int64_t i = 1; i <= n; ++i) {
        uint32_t left = INF;
        for (uint32_t t = 0; t < NB; ++t) {
            const int64_t jj = i + (int64_t)t - (int64_t)W;
            uint32_t v;
            if (jj < 0 || jj > m) {
                v = INF;
            } else if (jj == 0) {
                v = (uint32_t)i;
            } else {
                const uint32_t diag = scratch[t * stride];
                const uint32_t up = (t + 1 < NB) ? scratch[(t + 1) * stride] : INF;
                v = diag + (a[i - 1] != b[jj - 1] ? 1u : 0u);
                v = min(v, min(up, left) + 1);
                v = min(v, INF);
            }
            scratch[t * stride] = v;
            left = v;
        }
    }
    return min(scratch[(uint32_t)(dd + W) * stride], W + 1);
}

}  // namespace nmz
