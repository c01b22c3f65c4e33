// The counter-based draws shared by the loader (csrc/loader.hip) and the batch mixer (csrc/mix.hip): the keyed Feistel
// permutation with cycle walking and the exact fp64 uniform of a tagged hash.  Formulas: include/hwgat_hip.h, "hashes" of
// the device-resident clip store.  mix32 is the dropout hash of fused_ops.h.
#pragma once
#include "common.h"
#include "fused_ops.h"

// the smallest even b >= 2 with 2^b >= n (n <= 2^30: b <= 30)
__device__ __forceinline__ int feistel_bits(uint32_t n) {
    int b = 2;
    while (b < 30 && (1u << b) < n) b += 2;
    return b;
}
// four balanced Feistel rounds on 2 h bits, round function mix32 under key K + round
__device__ __forceinline__ uint32_t feistel(uint32_t K, int h, uint32_t x) {
    const uint32_t m = (1u << h) - 1u;
    uint32_t L = x >> h, R = x & m;
#pragma unroll
    for (uint32_t j = 0; j < 4; ++j) {
        const uint32_t t = L ^ (mix32(K + j, (uint64_t)R) & m);
        L = R;
        R = t;
    }
    return (L << h) | R;
}
// keyed bijection of [0, n) by cycle walking, x < n.  The bound is never reached (header: the walk follows the cycle
// through x, which returns to x after at most 2^b - n points outside [0, n)); the result is in [0, n) either way
__device__ __forceinline__ uint32_t perm(uint32_t K, uint32_t n, uint32_t x) {
    if (n <= 1u) return 0u;
    const int b = feistel_bits(n), h = b >> 1;
    const uint64_t bound = (1ull << b) - n + 1ull;
    uint32_t y = x;
    for (uint64_t w = 0; w < bound; ++w) {
        y = feistel(K, h, y);
        if (y < n) return y;
    }
    return x;
}

__device__ __forceinline__ double uniform01(uint32_t key, uint32_t tag, uint32_t i) {
    return ((double)mix32(key + tag, (uint64_t)i) + 0.5) * (1.0 / 4294967296.0);     // exact
}
