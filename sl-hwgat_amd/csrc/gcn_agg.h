// The graph aggregation of the two GCN baselines (stgcn_ops.hip, dgcn_ops.hip), stated once.  Activations are
// channels-last fp32, V <= VMAX joints; channel c belongs to group c mod G and a group has its own three V x V matrices
// M[k, g] (ST-GCN: G = 1).
//
//   agg_k<0>         out[f, w, c]      = sum_{k, v} M[k, g, v, w] y[f, v, k C + c]
//   agg_k<1>         dy[f, v, k C + c] = sum_w      M[k, g, v, w] d[f, w, c]
//   agg_da_k         ws[b][g][k][v][w] (32 x 32 slots) = sum over block b's frames and the channels of group g of
//                    y[f, v, k C + c] d[f, w, c]
//   agg_da_reduce_k  the sum over the P block images, FIN_PH phases of every FIN_PH-th image added in phase order
//
// A workgroup serves ONE group (blockIdx.y): its three matrices sit in LDS (12 KiB, whatever G is).  What differs between
// the two models is the matrix source `Src`, passed by value:
//   float Src::at(k, g, v, w, V)    the entry M[k, g, v, w] that fills the LDS matrix
//   float Src::grad(i, s)           what the reduce writes at flat index i = ((k G + g) V + v) V + w for the image sum s
//   bool  Src::kGrouped             false: the source has one matrix set (G is always 1), no grouped kernel is built for it
// and the cap on block images, which the entry point passes: with the fpb / P arithmetic of `agg_images` it fixes the
// summation order of the matrix gradient and therefore its bits.  No kernel here uses an atomic.
#pragma once
#include "common.h"

namespace {

constexpr int VMAX = 32;
constexpr int FIN_PH = 16;      // phases of the second level of every fixed-order reduction

inline int grid1(int64_t n) { return (int)((n + 255) / 256); }

// ONE: the input has one group, so neighbouring lanes hold neighbouring channels and the group arithmetic folds away
// (58 VGPRs against 72 in the forward direction, and measurably faster: profiles/gcn_unify_lab.txt)
template <int TRANS, bool ONE, class Src>
__global__ __launch_bounds__(256) void agg_k(const float* __restrict__ src, const Src m, float* __restrict__ dst, int64_t NT,
                                              int V, int C, int groups) {
    __shared__ float Ms[3 * VMAX * VMAX];
    const int G = ONE ? 1 : groups, g = ONE ? 0 : blockIdx.y, J = C / G;
    for (int q = threadIdx.x; q < 3 * VMAX * VMAX; q += 256) {
        const int k = q / (VMAX * VMAX), v = (q / VMAX) % VMAX, w = q % VMAX;
        Ms[q] = (v < V && w < V) ? m.at(k, g, v, w, V) : 0.f;
    }
    __syncthreads();
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= NT * J) return;
    const int64_t f = i / J;
    const int c = (int)(i % J) * G + g;
    if (TRANS == 0) {
        float acc[VMAX];
#pragma unroll
        for (int w = 0; w < VMAX; ++w) acc[w] = 0.f;
        const float* yp = src + f * V * 3 * C + c;
        for (int k = 0; k < 3; ++k)
            for (int v = 0; v < V; ++v) {
                const float val = yp[((int64_t)v * 3 + k) * C];
                const float* ar = Ms + (k * VMAX + v) * VMAX;
#pragma unroll
                for (int w = 0; w < VMAX; ++w) acc[w] = fmaf(ar[w], val, acc[w]);
            }
        float* op = dst + f * V * C + c;
#pragma unroll
        for (int w = 0; w < VMAX; ++w)
            if (w < V) op[(int64_t)w * C] = acc[w];
    } else {
        float d[VMAX];
        const float* dp = src + f * V * C + c;
#pragma unroll
        for (int w = 0; w < VMAX; ++w) d[w] = w < V ? dp[(int64_t)w * C] : 0.f;
        float* op = dst + f * V * 3 * C + c;
        for (int k = 0; k < 3; ++k)
            for (int v = 0; v < V; ++v) {
                const float* ar = Ms + (k * VMAX + v) * VMAX;
                float s = 0.f;
#pragma unroll
                for (int w = 0; w < VMAX; ++w) s = fmaf(ar[w], d[w], s);
                op[((int64_t)v * 3 + k) * C] = s;
            }
    }
}

// 32 channels of the group per pass; the last chunk of a group may be short (jn < 32)
__global__ __launch_bounds__(256) void agg_da_k(const float* __restrict__ y, const float* __restrict__ d,
                                                 float* __restrict__ ws, int64_t NT, int V, int C, int G, int64_t fpb) {
    __shared__ float Ys[VMAX][3][33];
    __shared__ float Ds[VMAX][33];
    const int tid = threadIdx.x, v = tid & 31, wq = tid >> 5;
    const int g = blockIdx.y, J = C / G;
    float acc[3][4];
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[k][j] = 0.f;
    const int64_t f0 = (int64_t)blockIdx.x * fpb, f1 = min(NT, f0 + fpb);
    for (int64_t f = f0; f < f1; ++f)
        for (int j0 = 0; j0 < J; j0 += 32) {
            const int jn = min(32, J - j0);
            __syncthreads();
            for (int q = tid; q < VMAX * 3 * 32; q += 256) {
                const int cc = q & 31, k = (q >> 5) % 3, vv = q / 96;
                Ys[vv][k][cc] = (vv < V && cc < jn) ? y[((f * V + vv) * 3 + k) * C + (int64_t)(j0 + cc) * G + g] : 0.f;
            }
            for (int q = tid; q < VMAX * 32; q += 256) {
                const int cc = q & 31, ww = q >> 5;
                Ds[ww][cc] = (ww < V && cc < jn) ? d[(f * V + ww) * C + (int64_t)(j0 + cc) * G + g] : 0.f;
            }
            __syncthreads();
#pragma unroll 4
            for (int cc = 0; cc < jn; ++cc) {
                float dv[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) dv[j] = Ds[wq * 4 + j][cc];
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const float yv = Ys[v][k][cc];
#pragma unroll
                    for (int j = 0; j < 4; ++j) acc[k][j] = fmaf(yv, dv[j], acc[k][j]);
                }
            }
        }
    float* img = ws + ((int64_t)blockIdx.x * G + g) * 3 * VMAX * VMAX;
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int j = 0; j < 4; ++j) img[(k * VMAX + v) * VMAX + wq * 4 + j] = acc[k][j];
}

template <class Src>
__global__ __launch_bounds__(64 * FIN_PH) void agg_da_reduce_k(const float* __restrict__ ws, int P, const Src m,
                                                                float* __restrict__ dM, int V, int G) {
    __shared__ float red[FIN_PH][64];
    const int cl = threadIdx.x & 63, ph = threadIdx.x >> 6;
    const int i = blockIdx.x * 64 + cl;
    const bool live = i < 3 * G * V * V;
    float s = 0.f;
    if (live) {
        const int w = i % V, v = (i / V) % V, g = (i / (V * V)) % G, k = i / (V * V * G);
        for (int p = ph; p < P; p += FIN_PH)
            s += ws[((int64_t)p * G + g) * 3 * VMAX * VMAX + (k * VMAX + v) * VMAX + w];
    }
    red[ph][cl] = s;
    __syncthreads();
    if (ph != 0 || !live) return;
    for (int q = 1; q < FIN_PH; ++q) s += red[q][cl];
    dM[i] = m.grad(i, s);
}

// P block images of fpb frames each, at most `cap` of them
inline int agg_images(int64_t NT, int cap, int64_t& fpb) {
    const int P = (int)(NT < cap ? NT : cap);
    fpb = (NT + P - 1) / P;
    return (int)((NT + fpb - 1) / fpb);
}

inline int64_t agg_bwd_bytes(int64_t NT, int G, int cap) {
    return (int64_t)(NT < cap ? NT : cap) * G * 3 * VMAX * VMAX * 4;
}

// the adjacency product in direction TRANS; G == 1 takes the one-group form, whichever model calls
template <int TRANS, class Src>
void agg_launch(const float* src, const Src& m, float* dst, int64_t NT, int V, int C, int G, hipStream_t st) {
    const dim3 grid(grid1(NT * (C / G)), G);
    if (G == 1) agg_k<TRANS, true><<<grid, 256, 0, st>>>(src, m, dst, NT, V, C, G);
    else if constexpr (Src::kGrouped) agg_k<TRANS, false><<<grid, 256, 0, st>>>(src, m, dst, NT, V, C, G);
}

// dy, and when dM the matrix gradient through ws (agg_bwd_bytes(NT, G, cap) bytes)
template <class Src>
void agg_bwd_launch(const float* y, const float* d, const Src& m, float* dy, float* dM, int64_t NT, int V, int C, int G,
                    int cap, float* ws, hipStream_t st) {
    agg_launch<1>(d, m, dy, NT, V, C, G, st);
    if (!dM) return;
    int64_t fpb;
    const int P = agg_images(NT, cap, fpb);
    agg_da_k<<<dim3(P, G), 256, 0, st>>>(y, d, ws, NT, V, C, G, fpb);
    agg_da_reduce_k<<<(3 * G * V * V + 63) / 64, 64 * FIN_PH, 0, st>>>(ws, P, m, dM, V, G);
}

}  // namespace
