// Score fusion of an ensemble for gfx950 (ensemble.Ensemble): the fp32 logits z (M, B, C) of M <= 8 members and M weights
// in DEVICE memory give one (B, C) score (formulas: include/hwgat_hip.h, "score ensemble").  The weights are read when the
// kernel runs, so a captured evaluation follows a new weight without a new capture.
//
//   ens_fuse_k<THREADS>   one workgroup of THREADS lanes per row b.
//     logit mode  out = sum_m w[m] z[m]: every product and every sum rounded to fp32 on its own, members in order from 0.0.
//     prob mode   out = log sum_m w[m] softmax(z[m]): per member the row maximum (fp32) and the sum of expf(z - max) kept in
//                 double give lse[m]; an entry is the log-sum-exp over the members of log w[m] + z[m] - lse[m], formed in
//                 double with the largest term taken out and rounded to fp32 once.  No probability is ever formed.  A
//                 member whose weight is not > 0 is not read.
//
// THREADS is 64 (one wave, no LDS, no barrier) for rows of up to ENS_WAVE_MAX_C classes and 256 above (the waves' partial
// results meet in a few LDS words): at M 4, B 64, C 2002 one wave per row takes 17.9 us (logit) / 64.5 us (prob), the
// workgroup 6.3 / 24.0 (tools/ensemble_lab.py, profiles/ensemble_lab.txt).  No float atomics: every word has one writer and
// every sum one order, so a repeat is bit-equal.  All stores are plain vector stores.
#include <math.h>
#include <stdlib.h>

#include "common.h"

namespace {

constexpr int ENS_WAVE_MAX_C = 512;

struct MaxOp { __device__ __forceinline__ float operator()(float a, float b) const { return fmaxf(a, b); } };
struct AddOp { __device__ __forceinline__ double operator()(double a, double b) const { return a + b; } };

// every lane gets the same bits: the butterfly pairs lanes symmetrically and both operations commute
template <int THREADS, class T, class Op>
__device__ __forceinline__ T row_reduce(T v, T* sh, Op op) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v = op(v, __shfl_xor(v, d, 64));
    if constexpr (THREADS > 64) {
        if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
        __syncthreads();
        T r = sh[0];
#pragma unroll
        for (int i = 1; i < THREADS / 64; ++i) r = op(r, sh[i]);
        __syncthreads();                                      // sh is free for the next reduction
        return r;
    }
    return v;
}

template <int THREADS>
__global__ __launch_bounds__(THREADS) void ens_fuse_k(const float* __restrict__ z, const float* __restrict__ w,
                                                      float* __restrict__ out, int M, int64_t B, int C, int mode) {
    __shared__ float sh_f[THREADS / 64];
    __shared__ double sh_d[THREADS / 64];
    const int64_t b = blockIdx.x;
    const int64_t plane = B * C;                              // floats between two members' rows
    const float* zb = z + b * C;
    float* ob = out + b * C;
    float wm[HWGAT_ENS_MAX_MEMBERS];
#pragma unroll
    for (int m = 0; m < HWGAT_ENS_MAX_MEMBERS; ++m) wm[m] = m < M ? w[m] : 0.f;

    if (mode == HWGAT_ENS_LOGIT) {
        for (int c = threadIdx.x; c < C; c += THREADS) {
            float acc = 0.f;
#pragma unroll
            for (int m = 0; m < HWGAT_ENS_MAX_MEMBERS; ++m)
                if (m < M) acc = __fadd_rn(acc, __fmul_rn(wm[m], zb[m * plane + c]));
            ob[c] = acc;
        }
        return;
    }

    // prob mode.  `on`, M and the trip counts are uniform in the workgroup: every lane reaches every barrier
    double shift[HWGAT_ENS_MAX_MEMBERS];                      // log w[m] - lse[m]
    bool on[HWGAT_ENS_MAX_MEMBERS];
#pragma unroll
    for (int m = 0; m < HWGAT_ENS_MAX_MEMBERS; ++m) {
        on[m] = m < M && wm[m] > 0.f;
        shift[m] = 0.0;
        if (!on[m]) continue;
        const float* zm = zb + m * plane;
        float mx = -INFINITY;
        for (int c = threadIdx.x; c < C; c += THREADS) mx = fmaxf(mx, zm[c]);
        mx = row_reduce<THREADS>(mx, sh_f, MaxOp{});
        double s = 0.0;
        for (int c = threadIdx.x; c < C; c += THREADS) s += (double)expf(__fsub_rn(zm[c], mx));   // a NaN entry lands here
        s = row_reduce<THREADS>(s, sh_d, AddOp{});
        shift[m] = log((double)wm[m]) - ((double)mx + log(s));
    }
    for (int c = threadIdx.x; c < C; c += THREADS) {
        double t[HWGAT_ENS_MAX_MEMBERS], top = -INFINITY;
        bool bad = false;
#pragma unroll
        for (int m = 0; m < HWGAT_ENS_MAX_MEMBERS; ++m) {
            t[m] = -INFINITY;
            if (!on[m]) continue;
            t[m] = (double)zb[m * plane + c] + shift[m];
            bad = bad || t[m] != t[m];
            top = fmax(top, t[m]);
        }
        double r;
        if (bad) {
            r = NAN;
        } else if (top == -INFINITY) {
            r = -INFINITY;                                    // every member gives the class probability 0 (or none is read)
        } else {
            double s = 0.0;
#pragma unroll
            for (int m = 0; m < HWGAT_ENS_MAX_MEMBERS; ++m)
                if (on[m]) s += exp(t[m] - top);              // the largest term is exp(0) = 1: s >= 1
            r = top + log(s);
        }
        ob[c] = (float)r;
    }
}

}  // namespace

extern "C" int hwgat_ens_fuse(const float* z, const float* w, float* out, int M, int B, int C, int mode, void* stream) {
    if (!z || !w || !out || B <= 0 || C <= 0) return HWGAT_EINVAL;
    if (M < 1 || M > HWGAT_ENS_MAX_MEMBERS) return HWGAT_ESHAPE;
    if (mode != HWGAT_ENS_LOGIT && mode != HWGAT_ENS_PROB) return HWGAT_ESHAPE;
    bool wave = C <= ENS_WAVE_MAX_C;
    if (const char* v = lab_env("HWGAT_ENS_THREADS")) wave = atoi(v) == 64;     // lab build only: the other size at any C
    if (wave)
        ens_fuse_k<64><<<B, 64, 0, (hipStream_t)stream>>>(z, w, out, M, B, C, mode);
    else
        ens_fuse_k<256><<<B, 256, 0, (hipStream_t)stream>>>(z, w, out, M, B, C, mode);
    HWGAT_LAUNCH_CHECK();
}
