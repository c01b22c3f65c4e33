// Row-wise kernels of the ST-GCN baseline (reference hwgat/models/STGCN.py) on channels-last activations: M rows of C
// floats, a BatchNorm channel is a column.
//
// BatchNorm    hwgat_stgcn_bn_stats: column statistics in two levels -- per-block partial sums of (x - k) and (x - k)^2
//              with the shift k = the column's first row (no E[x^2] - E[x]^2 cancellation), then one finalise kernel
//              that adds the partials in a fixed order (16 phases of every 16th image, then the phases; double),
//              writes mean / rstd, updates running_mean / running_var (unbiased) and num_batches_tracked on the device.  hwgat_stgcn_bn_apply: normalise (+ residual, itself
//              optionally normalised) (+ ReLU).  hwgat_stgcn_bn_bwd: g = dy [y > 0], column sums of g and g xhat in the
//              same two levels, then dx; d gamma / d beta written.
// aggregation  hwgat_stgcn_agg_fwd: out[f, w, c] = sum_{k,v} Ae[k, v, w] y[f, v, k C + c], Ae = A o edge_importance built
//              in LDS; one thread per (frame, channel), the V outputs in registers.  hwgat_stgcn_agg_bwd: the transposed
//              product for dy and the (3, V, V) gradient through per-block images added in block order.  The kernels are
//              gcn_agg.h's, shared with dgcn_ops.hip, at one group; this file states the matrix source (EdgeWeighted)
//              and the cap on block images.
// pool         mean over the T V rows of a clip, head dropout fused (mask index n C + c), and its backward.
// No kernel here uses an atomic: every cross-block sum is a fixed-order sum of partial images.
#include "common.h"
#include "fused_ops.h"
#include "gcn_agg.h"

namespace {

constexpr int RED_BLOCKS = 256;      // partial images of a column reduction
constexpr int AGG_BLOCKS = 512;      // cap on the block images of d edge_importance

enum { RED_STATS = 0, RED_BWD = 1, RED_SUM = 2 };

// ws[(p * 2 + j) * C + c]: block p's partial of sum j for column c
template <int MODE>
__global__ __launch_bounds__(256) void colred_k(const float* __restrict__ x, const float* __restrict__ dy,
                                                 const float* __restrict__ y, const float* __restrict__ mean,
                                                 const float* __restrict__ rstd, float* __restrict__ ws, int64_t M, int C,
                                                 int64_t chunk) {
    __shared__ float red[4][64][2];
    const int cl = threadIdx.x & 63, ph = threadIdx.x >> 6;
    const int c = blockIdx.x * 64 + cl;
    const int64_t r_begin = (int64_t)blockIdx.y * chunk, r_end = min(M, r_begin + chunk);
    float s1 = 0.f, s2 = 0.f;
    if (c < C) {
        float k0 = 0.f, k1 = 1.f;
        if (MODE == RED_STATS) k0 = x[c];
        if (MODE == RED_BWD) { k0 = mean[c]; k1 = rstd[c]; }
        for (int64_t r = r_begin + ph; r < r_end; r += 4) {
            const int64_t i = r * C + c;
            if (MODE == RED_STATS) {
                const float a = x[i] - k0;
                s1 += a;
                s2 = fmaf(a, a, s2);
            } else if (MODE == RED_BWD) {
                float g = dy[i];
                if (y && !(y[i] > 0.f)) g = 0.f;
                s1 += g;
                s2 = fmaf(g, (x[i] - k0) * k1, s2);
            } else {
                s1 += x[i];
            }
        }
    }
    red[ph][cl][0] = s1;
    red[ph][cl][1] = s2;
    __syncthreads();
    if (ph == 0 && c < C) {
        float a = red[0][cl][0], b = red[0][cl][1];
        for (int q = 1; q < 4; ++q) { a += red[q][cl][0]; b += red[q][cl][1]; }
        ws[((int64_t)blockIdx.y * 2 + 0) * C + c] = a;
        ws[((int64_t)blockIdx.y * 2 + 1) * C + c] = b;
    }
}

// Second level of a column reduction: one workgroup per 64 columns, FIN_PH phases each adding every FIN_PH-th partial
// image in double, the phases then added in phase order -- a fixed order, so the sums are bit-reproducible.  Returns
// true in the one thread per column that holds the two sums.
__device__ __forceinline__ bool fin_sums(const float* __restrict__ ws, int P, int C, int& c, double& s1, double& s2) {
    __shared__ double red[FIN_PH][64][2];
    const int cl = threadIdx.x & 63, ph = threadIdx.x >> 6;
    c = blockIdx.x * 64 + cl;
    double a = 0.0, b = 0.0;
    if (c < C)
        for (int p = ph; p < P; p += FIN_PH) {
            a += (double)ws[((int64_t)p * 2 + 0) * C + c];
            b += (double)ws[((int64_t)p * 2 + 1) * C + c];
        }
    red[ph][cl][0] = a;
    red[ph][cl][1] = b;
    __syncthreads();
    if (ph != 0 || c >= C) return false;
    for (int q = 1; q < FIN_PH; ++q) { a += red[q][cl][0]; b += red[q][cl][1]; }
    s1 = a;
    s2 = b;
    return true;
}

__global__ __launch_bounds__(64 * FIN_PH) void bn_stats_fin_k(const float* __restrict__ ws, int P, int C, int64_t M,
                                                               const float* __restrict__ x, float eps, float momentum,
                                                               float* __restrict__ mean, float* __restrict__ rstd,
                                                               float* __restrict__ rmean, float* __restrict__ rvar,
                                                               int64_t* __restrict__ nbt) {
    if (blockIdx.x == 0 && threadIdx.x == 0 && nbt) nbt[0] += 1;
    int c;
    double s1, s2;
    if (!fin_sums(ws, P, C, c, s1, s2)) return;
    const double m = s1 / (double)M;
    double var = s2 / (double)M - m * m;
    if (var < 0.0) var = 0.0;
    const double mu = (double)x[c] + m;
    mean[c] = (float)mu;
    rstd[c] = (float)(1.0 / sqrt(var + (double)eps));
    if (rmean) {
        rmean[c] = (float)((1.0 - (double)momentum) * (double)rmean[c] + (double)momentum * mu);
        rvar[c] = (float)((1.0 - (double)momentum) * (double)rvar[c] +
                          (double)momentum * var * ((double)M / (double)(M - 1)));
    }
}

// sums[c] = sum g, sums[C + c] = sum g xhat (also d beta, d gamma)
__global__ __launch_bounds__(64 * FIN_PH) void red_fin_k(const float* __restrict__ ws, int P, int C,
                                                          float* __restrict__ out0, float* __restrict__ out1,
                                                          float* __restrict__ sums) {
    int c;
    double s1, s2;
    if (!fin_sums(ws, P, C, c, s1, s2)) return;
    if (out0) out0[c] = (float)s1;
    if (out1) out1[c] = (float)s2;
    if (sums) { sums[c] = (float)s1; sums[C + c] = (float)s2; }
}

__global__ __launch_bounds__(256) void bn_dx_k(const float* __restrict__ dy, const float* __restrict__ y,
                                                const float* __restrict__ x, const float* __restrict__ mean,
                                                const float* __restrict__ rstd, const float* __restrict__ gamma,
                                                const float* __restrict__ sums, float* __restrict__ dx, int64_t n, int C,
                                                float inv_m) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int c = (int)(i % C);
    float g = dy[i];
    if (y && !(y[i] > 0.f)) g = 0.f;
    const float rs = rstd[c];
    if (sums) {                                   // batch statistics: the mean and the variance depend on x too
        const float xh = (x[i] - mean[c]) * rs;
        g -= (sums[c] + xh * sums[C + c]) * inv_m;
    }
    dx[i] = gamma[c] * rs * g;
}

__global__ __launch_bounds__(256) void bn_apply_k(const float* __restrict__ x, const float* __restrict__ mean,
                                                   const float* __restrict__ rstd, const float* __restrict__ gamma,
                                                   const float* __restrict__ beta, const float* __restrict__ res,
                                                   const float* __restrict__ rmean, const float* __restrict__ rrstd,
                                                   const float* __restrict__ rgamma, const float* __restrict__ rbeta,
                                                   float* __restrict__ out, int64_t n, int C, int relu) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int c = (int)(i % C);
    float v = (x[i] - mean[c]) * rstd[c] * gamma[c] + beta[c];
    if (res) {
        float r = res[i];
        if (rmean) r = (r - rmean[c]) * rrstd[c] * rgamma[c] + rbeta[c];
        v += r;
    }
    out[i] = relu ? fmaxf(v, 0.f) : v;
}

__global__ __launch_bounds__(256) void bn_eval_stats_k(const float* __restrict__ rm, const float* __restrict__ rv,
                                                        float eps, float* __restrict__ mean, float* __restrict__ rstd,
                                                        int C) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    mean[c] = rm[c];
    rstd[c] = (float)(1.0 / sqrt((double)rv[c] + (double)eps));
}

// the ST-GCN matrix source of gcn_agg.h: M = A o edge_importance (E null: ones), one group; the gradient is dE = A . s
struct EdgeWeighted {
    static constexpr bool kGrouped = false;
    const float* A;
    const float* E;
    __device__ float at(int k, int, int v, int w, int V) const {
        const int i = (k * V + v) * V + w;
        return A[i] * (E ? E[i] : 1.f);
    }
    __device__ float grad(int i, float s) const { return A[i] * s; }
};

__global__ __launch_bounds__(256) void pool_fwd_k(const float* __restrict__ x, float* __restrict__ out, int R, int C,
                                                   uint32_t seed, float p, const uint32_t* seed_base) {
    __shared__ float red[4][64];
    const int cl = threadIdx.x & 63, ph = threadIdx.x >> 6;
    const int n = blockIdx.x, c = blockIdx.y * 64 + cl;
    float s = 0.f;
    if (c < C) {
        const float* xp = x + (int64_t)n * R * C + c;
        for (int r = ph; r < R; r += 4) s += xp[(int64_t)r * C];
    }
    red[ph][cl] = s;
    __syncthreads();
    if (ph == 0 && c < C) {
        float v = ((red[0][cl] + red[1][cl]) + (red[2][cl] + red[3][cl])) / (float)R;
        const uint32_t th = drop_thresh(p);
        if (th) v *= drop_keep(seed + seed_base_of(seed_base), (uint64_t)((int64_t)n * C + c), th, 1.0f / (1.0f - p));
        out[(int64_t)n * C + c] = v;
    }
}

__global__ __launch_bounds__(256) void pool_bwd_k(const float* __restrict__ dout, float* __restrict__ dx, int64_t total,
                                                   int R, int C, uint32_t seed, float p, const uint32_t* seed_base) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int c = (int)(i % C);
    const int64_t o = (i / C / R) * C + c;
    float v = dout[o] / (float)R;
    const uint32_t th = drop_thresh(p);
    if (th) v *= drop_keep(seed + seed_base_of(seed_base), (uint64_t)o, th, 1.0f / (1.0f - p));
    dx[i] = v;
}

__global__ __launch_bounds__(256) void copy_cols_k(const float* __restrict__ src, int lds, float* __restrict__ dst, int ldd,
                                                    int64_t total) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int c = (int)(i % ldd);
    dst[i] = c < lds ? src[(i / ldd) * lds + c] : 0.f;
}

int red_launch(int mode, const float* x, const float* dy, const float* y, const float* mean, const float* rstd, float* ws,
               int64_t M, int C, hipStream_t st) {
    int P = (int)((M + 63) / 64 < RED_BLOCKS ? (M + 63) / 64 : RED_BLOCKS);
    const int64_t chunk = (M + P - 1) / P;
    P = (int)((M + chunk - 1) / chunk);
    const dim3 grid((C + 63) / 64, P);
    if (mode == RED_STATS) colred_k<RED_STATS><<<grid, 256, 0, st>>>(x, dy, y, mean, rstd, ws, M, C, chunk);
    else if (mode == RED_BWD) colred_k<RED_BWD><<<grid, 256, 0, st>>>(x, dy, y, mean, rstd, ws, M, C, chunk);
    else colred_k<RED_SUM><<<grid, 256, 0, st>>>(x, dy, y, mean, rstd, ws, M, C, chunk);
    return P;
}

}  // namespace

extern "C" int64_t hwgat_stgcn_red_bytes(int C) {
    if (C <= 0) return -1;
    return ((int64_t)RED_BLOCKS * 2 * C + 2 * C) * 4;
}

extern "C" int hwgat_stgcn_colsum(const float* x, float* out, int64_t M, int C, float* ws, int64_t ws_bytes, void* stream) {
    if (!x || !out || !ws || M <= 0 || C <= 0 || ws_bytes < hwgat_stgcn_red_bytes(C)) return HWGAT_EINVAL;
    if (M * C / 256 > 0x7fffffff) return HWGAT_ESHAPE;
    hipStream_t st = (hipStream_t)stream;
    const int P = red_launch(RED_SUM, x, nullptr, nullptr, nullptr, nullptr, ws, M, C, st);
    red_fin_k<<<(C + 63) / 64, 64 * FIN_PH, 0, st>>>(ws, P, C, out, nullptr, nullptr);
    HWGAT_LAUNCH_CHECK();
}

extern "C" int hwgat_stgcn_bn_stats(const float* x, int64_t M, int C, float eps, float momentum, float* mean, float* rstd,
                                    float* running_mean, float* running_var, int64_t* num_batches, float* ws,
                                    int64_t ws_bytes, void* stream) {
    if (!x || !mean || !rstd || !ws || C <= 0 || M <= 0 || ws_bytes < hwgat_stgcn_red_bytes(C)) return HWGAT_EINVAL;
    if ((running_mean == nullptr) != (running_var == nullptr)) return HWGAT_EINVAL;
    if (M < 2 || M * C / 256 > 0x7fffffff) return HWGAT_ESHAPE;       // one value per channel: torch refuses it too
    hipStream_t st = (hipStream_t)stream;
    const int P = red_launch(RED_STATS, x, nullptr, nullptr, nullptr, nullptr, ws, M, C, st);
    bn_stats_fin_k<<<(C + 63) / 64, 64 * FIN_PH, 0, st>>>(ws, P, C, M, x, eps, momentum, mean, rstd, running_mean, running_var,
                                            num_batches);
    HWGAT_LAUNCH_CHECK();
}

extern "C" int hwgat_stgcn_bn_eval_stats(const float* rm, const float* rv, float eps, float* mean, float* rstd, int C,
                                         void* stream) {
    if (!rm || !rv || !mean || !rstd || C <= 0) return HWGAT_EINVAL;
    bn_eval_stats_k<<<grid1(C), 256, 0, (hipStream_t)stream>>>(rm, rv, eps, mean, rstd, C);
    HWGAT_LAUNCH_CHECK();
}

extern "C" int hwgat_stgcn_bn_apply(const float* x, const float* mean, const float* rstd, const float* gamma,
                                    const float* beta, const float* res, const float* res_mean, const float* res_rstd,
                                    const float* res_gamma, const float* res_beta, float* out, int64_t M, int C, int relu,
                                    void* stream) {
    if (!x || !mean || !rstd || !gamma || !beta || !out || M <= 0 || C <= 0) return HWGAT_EINVAL;
    if (res_mean && (!res || !res_rstd || !res_gamma || !res_beta)) return HWGAT_EINVAL;
    if (M * C / 256 > 0x7fffffff) return HWGAT_ESHAPE;
    bn_apply_k<<<grid1(M * C), 256, 0, (hipStream_t)stream>>>(x, mean, rstd, gamma, beta, res, res_mean, res_rstd,
                                                             res_gamma, res_beta, out, M * C, C, relu);
    HWGAT_LAUNCH_CHECK();
}

extern "C" int hwgat_stgcn_bn_bwd(const float* dy, const float* y, const float* x, const float* mean, const float* rstd,
                                  const float* gamma, float* dx, float* dgamma, float* dbeta, int64_t M, int C, int train,
                                  float* ws, int64_t ws_bytes, void* stream) {
    if (!dy || !x || !mean || !rstd || !gamma || !dx || !dgamma || !dbeta || !ws || M <= 0 || C <= 0) return HWGAT_EINVAL;
    if (ws_bytes < hwgat_stgcn_red_bytes(C)) return HWGAT_EINVAL;
    if (M * C / 256 > 0x7fffffff) return HWGAT_ESHAPE;
    hipStream_t st = (hipStream_t)stream;
    float* sums = ws + (int64_t)RED_BLOCKS * 2 * C;
    const int P = red_launch(RED_BWD, x, dy, y, mean, rstd, ws, M, C, st);
    red_fin_k<<<(C + 63) / 64, 64 * FIN_PH, 0, st>>>(ws, P, C, dbeta, dgamma, sums);
    bn_dx_k<<<grid1(M * C), 256, 0, st>>>(dy, y, x, mean, rstd, gamma, train ? sums : nullptr, dx, M * C, C,
                                         1.0f / (float)M);
    HWGAT_LAUNCH_CHECK();
}

extern "C" int hwgat_stgcn_agg_fwd(const float* y, const float* A, const float* E, float* out, int64_t NT, int V, int C,
                                   void* stream) {
    if (!y || !A || !out || NT <= 0 || C <= 0) return HWGAT_EINVAL;
    if (V <= 0 || V > VMAX || NT * C / 256 > 0x7fffffff) return HWGAT_ESHAPE;
    agg_launch<0>(y, EdgeWeighted{A, E}, out, NT, V, C, 1, (hipStream_t)stream);
    HWGAT_LAUNCH_CHECK();
}

extern "C" int64_t hwgat_stgcn_agg_bwd_bytes(int64_t NT) {
    if (NT <= 0) return -1;
    return agg_bwd_bytes(NT, 1, AGG_BLOCKS);
}

extern "C" int hwgat_stgcn_agg_bwd(const float* y, const float* d, const float* A, const float* E, float* dy, float* dE,
                                   int64_t NT, int V, int C, float* ws, int64_t ws_bytes, void* stream) {
    if (!y || !d || !A || !dy || NT <= 0 || C <= 0) return HWGAT_EINVAL;
    if (dE && (!ws || ws_bytes < hwgat_stgcn_agg_bwd_bytes(NT))) return HWGAT_EINVAL;
    if (V <= 0 || V > VMAX || C % 32 || NT * C / 256 > 0x7fffffff) return HWGAT_ESHAPE;
    agg_bwd_launch(y, d, EdgeWeighted{A, E}, dy, dE, NT, V, C, 1, AGG_BLOCKS, ws, (hipStream_t)stream);
    HWGAT_LAUNCH_CHECK();
}

extern "C" int hwgat_stgcn_pool_fwd(const float* x, float* out, int N, int R, int C, uint32_t seed, float p,
                                    const uint32_t* seed_base, void* stream) {
    if (!x || !out || N <= 0 || R <= 0 || C <= 0 || p < 0.f || p >= 1.f) return HWGAT_EINVAL;
    pool_fwd_k<<<dim3(N, (C + 63) / 64), 256, 0, (hipStream_t)stream>>>(x, out, R, C, seed, p, seed_base);
    HWGAT_LAUNCH_CHECK();
}

extern "C" int hwgat_stgcn_pool_bwd(const float* dout, float* dx, int N, int R, int C, uint32_t seed, float p,
                                    const uint32_t* seed_base, void* stream) {
    if (!dout || !dx || N <= 0 || R <= 0 || C <= 0 || p < 0.f || p >= 1.f) return HWGAT_EINVAL;
    const int64_t total = (int64_t)N * R * C;
    if (total / 256 > 0x7fffffff) return HWGAT_ESHAPE;
    pool_bwd_k<<<grid1(total), 256, 0, (hipStream_t)stream>>>(dout, dx, total, R, C, seed, p, seed_base);
    HWGAT_LAUNCH_CHECK();
}

extern "C" int hwgat_stgcn_copy_cols(const float* src, int ld_src, float* dst, int ld_dst, int64_t rows, void* stream) {
    if (!src || !dst || ld_src <= 0 || ld_dst <= 0 || rows <= 0) return HWGAT_EINVAL;
    const int64_t total = rows * ld_dst;
    if (total / 256 > 0x7fffffff) return HWGAT_ESHAPE;
    copy_cols_k<<<grid1(total), 256, 0, (hipStream_t)stream>>>(src, ld_src, dst, ld_dst, total);
    HWGAT_LAUNCH_CHECK();
}
