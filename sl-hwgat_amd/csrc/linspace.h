// numpy.linspace(0, last, n).astype(int)[i] on the device, shared by stream.hip (TemporalSample of a live window) and
// loader.hip (TemporalAugmentation and TemporalSample of a train clip).
#pragma once
#include "common.h"

// numpy computes arange(n) * (last / (n - 1)) in fp64 and then sets the last entry to `last`: a separately rounded
// quotient and product (no FMA), truncated.  n <= 1: linspace(0, last, 1) = [0].  The result is reduced to [0, last].
__device__ __forceinline__ int linspace_int(int i, int last, int n) {
    if (n <= 1 || last <= 0) return 0;
    const double step = __ddiv_rn((double)last, (double)(n - 1));
    return i >= n - 1 ? last : min(max((int)__dmul_rn((double)i, step), 0), last);
}
