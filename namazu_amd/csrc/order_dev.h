// delay = h mod m of the replayable policy's release times (replayablepolicy.go:100-126), by the class of m: shared
// by the order sweep (order.hip) and the delivery sweep (delivery.hip).
#pragma once
#include "nmz_common.h"

namespace nmz {

// how delay = h mod m is reduced
enum : int {
    ORD_ZERO = 0,   // m == 0: every delay is 0 (replayablepolicy.go:101-104)
    ORD_SMALL = 1,  // 0 < m < 2^31: mod_barrett_small
    ORD_MID = 2,    // 2^31 <= m < 2^32: mod_barrett64
    ORD_WIDE = 3    // m >= 2^32: the same estimate with a 64-bit remainder
};

inline int order_kind(uint64_t m) {
    return m == 0 ? ORD_ZERO : m < (1ull << 31) ? ORD_SMALL : m < (1ull << 32) ? ORD_MID : ORD_WIDE;
}

// floor(2^64 / m), 2^64 - 1 for m = 1 (make_mod's mu, for every m > 0)
inline uint64_t order_mu(uint64_t m) {
    return m <= 1 ? ~0ull : (uint64_t)(((unsigned __int128)1 << 64) / m);
}

// v mod m. ORD_WIDE: q = floor(v * mu / 2^64) is floor(v / m) or one less (v * mu / 2^64 > v / m - 1), so
// r = v - q m < 2 m <= 2^62 and one conditional subtract finishes, as in mod_barrett64.
template <int KIND>
__device__ __forceinline__ uint64_t order_mod(uint64_t v, uint64_t m, uint64_t mu) {
    if (KIND == ORD_SMALL) return mod_barrett_small(v, (uint32_t)m, mu);
    if (KIND == ORD_MID) return mod_barrett64(v, m, mu);
    const uint64_t r = v - umulhi64(v, mu) * m;
    return r >= m ? r - m : r;
}

}  // namespace nmz
