// Kernels of the DecoupledGCN baseline (reference hwgat/models/DecoupledGCN.py) that the ST-GCN set does not have, on
// channels-last fp32 activations (N, T, V, C), V <= 32:
//
// aggregation  hwgat_dgcn_agg_fwd / _bwd: the per-channel-group adjacency product.  A workgroup serves ONE group g
//              (blockIdx.y): its three V x V matrices sit in LDS (12 KiB, whatever G is) and its threads walk the
//              (frame, channel c = j G + g) pairs, the V outputs of a pair in registers.  d An through per-block images
//              added in block order (16 phases of every 16th image, then the phases).  The kernels are gcn_agg.h's,
//              shared with stgcn_ops.hip; this file states the matrix source (GroupTable) and the cap on block images.
// gates        hwgat_dgcn_gate_sum: the squeezes (and, in the backward, the gate gradients) as sums over t or over v with
//              the gate factors applied while reading; 64 channels x 4 phases per workgroup, phases added in order.
//              hwgat_dgcn_gate_apply / _bwd: element-wise.
// DropGraph    hwgat_dgcn_abs_sum (the |x| statistic, BatchNorm and the earlier mask factor applied while reading),
//              hwgat_dgcn_draw (hash Bernoulli), hwgat_dgcn_mask_spatial / _temporal (one workgroup: mask and the
//              batch-wide normaliser, an integer count), hwgat_dgcn_merge / _merge_bwd.
// No kernel here uses an atomic.
#include "common.h"
#include "fused_ops.h"
#include "gcn_agg.h"

namespace {

constexpr int DA_BLOCKS = 128;      // cap on the frame chunks of d An (times G workgroups)

// the DecoupledGCN matrix source of gcn_agg.h: M[k, g] = An[k, g] of (3, G, V, V); the gradient is the image sum itself
struct GroupTable {
    static constexpr bool kGrouped = true;
    const float* An;
    int G;
    __device__ float at(int k, int g, int v, int w, int V) const { return An[(((int64_t)k * G + g) * V + v) * V + w]; }
    __device__ float grad(int, float s) const { return s; }
};

// AXIS 0: out[n, v, c] = scale sum_t val;  AXIS 1: out[n, t, c] = scale sum_v val
// val = h (g' (1 + sv[n, v]) (1 + st[n, t]) (1 + sc[n, c]) + m[n, t, c] m_scale)
template <int AXIS>
__global__ __launch_bounds__(256) void gate_sum_k(const float* __restrict__ h, const float* __restrict__ g,
                                                   const float* __restrict__ sv, const float* __restrict__ st,
                                                   const float* __restrict__ sc, const float* __restrict__ m, float m_scale,
                                                   float* __restrict__ out, int T, int V, int C, float scale) {
    __shared__ double red[4][64];
    const int cl = threadIdx.x & 63, ph = threadIdx.x >> 6;
    const int c = blockIdx.y * 64 + cl;
    const int row = blockIdx.x, D = AXIS == 0 ? V : T, L = AXIS == 0 ? T : V;
    const int n = row / D, o = row % D;
    double s = 0.0;                      // the sums feed gate gradients that cancel heavily: accumulate in double (free in a
    if (c < C) {                         // kernel that waits on memory)
        const float fc = sc ? 1.f + sc[(int64_t)n * C + c] : 1.f;
        for (int r = ph; r < L; r += 4) {
            const int t = AXIS == 0 ? r : o, v = AXIS == 0 ? o : r;
            const int64_t idx = (((int64_t)n * T + t) * V + v) * C + c;
            float w = fc;
            if (sv) w *= 1.f + sv[n * V + v];
            if (st) w *= 1.f + st[n * T + t];
            if (g) w *= g[idx];
            if (m) w = fmaf(m[((int64_t)n * T + t) * C + c], m_scale, w);
            s += (double)h[idx] * (double)w;
        }
    }
    red[ph][cl] = s;
    __syncthreads();
    if (ph == 0 && c < C)
        out[(int64_t)row * C + c] = (float)((double)scale * ((red[0][cl] + red[1][cl]) + (red[2][cl] + red[3][cl])));
}

// BWD 0: out = h (1 + sv)(1 + st)(1 + sc);  BWD 1: out = d (1 + sv)(1 + st)(1 + sc) + dm1[n, t, c] (1 + sv) / V + dm0[n, v, c] / T
template <int BWD>
__global__ __launch_bounds__(256) void gate_apply_k(const float* __restrict__ x, const float* __restrict__ sv,
                                                     const float* __restrict__ st, const float* __restrict__ sc,
                                                     const float* __restrict__ dm1, const float* __restrict__ dm0,
                                                     float* __restrict__ out, int64_t total, int T, int V, int C) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int c = (int)(i % C);
    const int64_t row = i / C;
    const int v = (int)(row % V);
    const int64_t nt = row / V;
    const int64_t n = nt / T;
    const float a = sv ? 1.f + sv[n * V + v] : 1.f;
    float w = a;
    if (st) w *= 1.f + st[nt];
    if (sc) w *= 1.f + sc[n * C + c];
    float r = x[i] * w;
    if (BWD) {
        if (dm1) r = fmaf(dm1[nt * C + c] * a, 1.f / (float)V, r);
        if (dm0) r = fmaf(dm0[(n * V + v) * C + c], 1.f / (float)T, r);
    }
    out[i] = r;
}

// fixed-order sum of one value per thread over the 256 threads of a workgroup (every thread gets the result)
__device__ __forceinline__ float block_sum(float s, float* red) {
    red[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    const float r = red[0];
    __syncthreads();
    return r;
}

// AXIS 0: out[n, v] = sum_{t, c} |z|;  AXIS 1: out[n, t] = sum_{v, c} |z| fs[n, v]
template <int AXIS>
__global__ __launch_bounds__(256) void abs_sum_k(const float* __restrict__ x, const float* __restrict__ mean,
                                                  const float* __restrict__ rstd, const float* __restrict__ gamma,
                                                  const float* __restrict__ beta, const float* __restrict__ fs,
                                                  float* __restrict__ out, int T, int V, int C) {
    __shared__ float red[256];
    const int row = blockIdx.x, D = AXIS == 0 ? V : T, L = AXIS == 0 ? T : V;
    const int n = row / D, o = row % D;
    float s = 0.f;
    for (int q = threadIdx.x; q < L * C; q += 256) {
        const int r = q / C, c = q % C;
        const int t = AXIS == 0 ? r : o, v = AXIS == 0 ? o : r;
        float z = x[(((int64_t)n * T + t) * V + v) * C + c];
        if (mean) z = (z - mean[c]) * rstd[c] * gamma[c] + beta[c];
        z = fabsf(z);
        if (AXIS == 1 && fs) z *= fs[n * V + v];
        s += z;
    }
    s = block_sum(s, red);
    if (threadIdx.x == 0) out[row] = s;
}

__global__ __launch_bounds__(256) void draw_k(const float* __restrict__ p, float* __restrict__ out, int64_t n, uint32_t seed,
                                               const uint32_t* seed_base) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float u = (float)(mix32(seed + seed_base_of(seed_base), (uint64_t)i) >> 8) * (1.0f / 16777216.0f);   // [0, 1)
    out[i] = u < p[i] ? 1.f : 0.f;
}

__device__ __forceinline__ int block_count(int s, int* red) {
    red[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    return red[0];
}

// one workgroup.  SPATIAL: hit[n, w] = sum_v seeds[n, v] A[v, w] > 0.001;  else hit[n, t] = any seed within block / 2 frames
template <int SPATIAL>
__global__ __launch_bounds__(256) void mask_k(const float* __restrict__ seeds, const float* __restrict__ A,
                                               float* __restrict__ f, float* __restrict__ scale_out, int N, int D, int block) {
    __shared__ float As[VMAX * VMAX];
    __shared__ int red[256];
    if (SPATIAL) {
        for (int q = threadIdx.x; q < D * D; q += 256) As[q] = A[q];
        __syncthreads();
    }
    const int total = N * D, half = block / 2;
    int live = 0;
    for (int i = threadIdx.x; i < total; i += 256) {
        const int n = i / D, o = i % D;
        bool hit = false;
        if (SPATIAL) {
            float m = 0.f;
            for (int v = 0; v < D; ++v) m = fmaf(seeds[n * D + v], As[v * D + o], m);
            hit = m > 0.001f;
        } else {
            const int lo = max(0, o - half), hi = min(D - 1, o + half);
            for (int t = lo; t <= hi; ++t) hit = hit || seeds[n * D + t] > 0.f;
        }
        f[i] = hit ? 0.f : 1.f;
        live += hit ? 0 : 1;
    }
    live = block_count(live, red);
    const float scale = (float)total / (float)live;
    for (int i = threadIdx.x; i < total; i += 256) f[i] *= scale;      // a thread rescales what it wrote itself
    if (threadIdx.x == 0) scale_out[0] = scale;
}

__global__ __launch_bounds__(256) void merge_k(const float* __restrict__ x, const float* __restrict__ mean,
                                                const float* __restrict__ rstd, const float* __restrict__ gamma,
                                                const float* __restrict__ beta, const float* __restrict__ res,
                                                const float* __restrict__ rmean, const float* __restrict__ rrstd,
                                                const float* __restrict__ rgamma, const float* __restrict__ rbeta,
                                                const float* __restrict__ fs1, const float* __restrict__ ft1,
                                                const float* __restrict__ fs2, const float* __restrict__ ft2,
                                                float* __restrict__ out, int64_t total, int T, int V, int C) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int c = (int)(i % C);
    const int64_t row = i / C;
    const int v = (int)(row % V);
    const int64_t nt = row / V, nv = (nt / T) * V + v;
    float a = (x[i] - mean[c]) * rstd[c] * gamma[c] + beta[c];
    float r = res[i];
    if (rmean) r = (r - rmean[c]) * rrstd[c] * rgamma[c] + rbeta[c];
    out[i] = fmaxf(fmaf(a, fs1[nv] * ft1[nt], r * (fs2[nv] * ft2[nt])), 0.f);
}

__global__ __launch_bounds__(256) void merge_bwd_k(const float* __restrict__ dout, const float* __restrict__ out,
                                                    const float* __restrict__ fs1, const float* __restrict__ ft1,
                                                    const float* __restrict__ fs2, const float* __restrict__ ft2,
                                                    float* __restrict__ dz1, float* __restrict__ dz2, int64_t total, int T,
                                                    int V, int C) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int64_t row = i / C;
    const int v = (int)(row % V);
    const int64_t nt = row / V, nv = (nt / T) * V + v;
    const float g = out[i] > 0.f ? dout[i] : 0.f;
    dz1[i] = g * (fs1[nv] * ft1[nt]);
    dz2[i] = g * (fs2[nv] * ft2[nt]);
}

__global__ __launch_bounds__(256) void masked_sum_k(const float* __restrict__ a, const float* __restrict__ ma,
                                                     const float* __restrict__ b, const float* __restrict__ mb,
                                                     float* __restrict__ out, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float x = a[i], y = b[i];
    if (ma && !(ma[i] > 0.f)) x = 0.f;
    if (mb && !(mb[i] > 0.f)) y = 0.f;
    out[i] = x + y;
}

inline bool bad_shape(int N, int T, int V, int C) {
    return V > VMAX || (int64_t)N * T * V * C / 256 > 0x7fffffff || (int64_t)N * T > 0x7fffffff ||
           (int64_t)N * (T > V ? T : V) * C > 0x7fffffff;
}

}  // namespace

extern "C" int hwgat_dgcn_agg_fwd(const float* y, const float* An, float* out, int64_t NT, int V, int C, int G,
                                  void* stream) {
    if (!y || !An || !out || NT <= 0 || C <= 0 || V <= 0 || G <= 0) return HWGAT_EINVAL;
    if (V > VMAX || C % G || G > 65535 || NT * (C / G) / 256 > 0x7fffffff) return HWGAT_ESHAPE;
    agg_launch<0>(y, GroupTable{An, G}, out, NT, V, C, G, (hipStream_t)stream);
    HWGAT_LAUNCH_CHECK();
}

extern "C" int64_t hwgat_dgcn_agg_bwd_bytes(int64_t NT, int G) {
    if (NT <= 0 || G <= 0) return -1;
    return agg_bwd_bytes(NT, G, DA_BLOCKS);
}

extern "C" int hwgat_dgcn_agg_bwd(const float* y, const float* d, const float* An, float* dy, float* dAn, int64_t NT, int V,
                                  int C, int G, float* ws, int64_t ws_bytes, void* stream) {
    if (!y || !d || !An || !dy || NT <= 0 || C <= 0 || V <= 0 || G <= 0) return HWGAT_EINVAL;
    if (dAn && (!ws || ws_bytes < hwgat_dgcn_agg_bwd_bytes(NT, G))) return HWGAT_EINVAL;
    if (V > VMAX || C % G || G > 65535 || NT * (C / G) / 256 > 0x7fffffff) return HWGAT_ESHAPE;
    agg_bwd_launch(y, d, GroupTable{An, G}, dy, dAn, NT, V, C, G, DA_BLOCKS, ws, (hipStream_t)stream);
    HWGAT_LAUNCH_CHECK();
}

extern "C" int hwgat_dgcn_gate_sum(const float* h, const float* g, const float* sv, const float* st, const float* sc,
                                   const float* m, float m_scale, float* out, int N, int T, int V, int C, int axis,
                                   float scale, void* stream) {
    if (!h || !out || N <= 0 || T <= 0 || V <= 0 || C <= 0 || (axis != 0 && axis != 1)) return HWGAT_EINVAL;
    if (bad_shape(N, T, V, C)) return HWGAT_ESHAPE;
    const dim3 grid(N * (axis == 0 ? V : T), (C + 63) / 64);
    if (grid.y > 65535) return HWGAT_ESHAPE;
    if (axis == 0) gate_sum_k<0><<<grid, 256, 0, (hipStream_t)stream>>>(h, g, sv, st, sc, m, m_scale, out, T, V, C, scale);
    else gate_sum_k<1><<<grid, 256, 0, (hipStream_t)stream>>>(h, g, sv, st, sc, m, m_scale, out, T, V, C, scale);
    HWGAT_LAUNCH_CHECK();
}

extern "C" int hwgat_dgcn_gate_apply(const float* h, const float* sv, const float* st, const float* sc, float* out, int N,
                                     int T, int V, int C, void* stream) {
    if (!h || !out || N <= 0 || T <= 0 || V <= 0 || C <= 0) return HWGAT_EINVAL;
    if (bad_shape(N, T, V, C)) return HWGAT_ESHAPE;
    const int64_t total = (int64_t)N * T * V * C;
    gate_apply_k<0><<<grid1(total), 256, 0, (hipStream_t)stream>>>(h, sv, st, sc, nullptr, nullptr, out, total, T, V, C);
    HWGAT_LAUNCH_CHECK();
}

extern "C" int hwgat_dgcn_gate_bwd(const float* d, const float* sv, const float* st, const float* sc, const float* dm1,
                                   const float* dm0, float* dh, int N, int T, int V, int C, void* stream) {
    if (!d || !dh || N <= 0 || T <= 0 || V <= 0 || C <= 0) return HWGAT_EINVAL;
    if (bad_shape(N, T, V, C)) return HWGAT_ESHAPE;
    const int64_t total = (int64_t)N * T * V * C;
    gate_apply_k<1><<<grid1(total), 256, 0, (hipStream_t)stream>>>(d, sv, st, sc, dm1, dm0, dh, total, T, V, C);
    HWGAT_LAUNCH_CHECK();
}

extern "C" int hwgat_dgcn_abs_sum(const float* x, const float* mean, const float* rstd, const float* gamma,
                                  const float* beta, const float* fs, float* out, int N, int T, int V, int C, int axis,
                                  void* stream) {
    if (!x || !out || N <= 0 || T <= 0 || V <= 0 || C <= 0 || (axis != 0 && axis != 1)) return HWGAT_EINVAL;
    if (mean && (!rstd || !gamma || !beta)) return HWGAT_EINVAL;
    if (bad_shape(N, T, V, C)) return HWGAT_ESHAPE;
    const int rows = N * (axis == 0 ? V : T);
    if (axis == 0) abs_sum_k<0><<<rows, 256, 0, (hipStream_t)stream>>>(x, mean, rstd, gamma, beta, fs, out, T, V, C);
    else abs_sum_k<1><<<rows, 256, 0, (hipStream_t)stream>>>(x, mean, rstd, gamma, beta, fs, out, T, V, C);
    HWGAT_LAUNCH_CHECK();
}

extern "C" int hwgat_dgcn_draw(const float* p, float* out, int64_t n, uint32_t seed, const uint32_t* seed_base,
                               void* stream) {
    if (!p || !out || n <= 0) return HWGAT_EINVAL;
    if (n / 256 > 0x7fffffff) return HWGAT_ESHAPE;
    draw_k<<<grid1(n), 256, 0, (hipStream_t)stream>>>(p, out, n, seed, seed_base);
    HWGAT_LAUNCH_CHECK();
}

extern "C" int hwgat_dgcn_mask_spatial(const float* seeds, const float* A, float* f, float* scale, int N, int V,
                                       void* stream) {
    if (!seeds || !A || !f || !scale || N <= 0 || V <= 0) return HWGAT_EINVAL;
    if (V > VMAX || (int64_t)N * V > 0x7fffffff) return HWGAT_ESHAPE;
    mask_k<1><<<1, 256, 0, (hipStream_t)stream>>>(seeds, A, f, scale, N, V, 0);
    HWGAT_LAUNCH_CHECK();
}

extern "C" int hwgat_dgcn_mask_temporal(const float* seeds, float* f, float* scale, int N, int T, int block, void* stream) {
    if (!seeds || !f || !scale || N <= 0 || T <= 0 || block <= 0) return HWGAT_EINVAL;
    if (block % 2 == 0 || (int64_t)N * T > 0x7fffffff) return HWGAT_ESHAPE;
    mask_k<0><<<1, 256, 0, (hipStream_t)stream>>>(seeds, nullptr, f, scale, N, T, block);
    HWGAT_LAUNCH_CHECK();
}

extern "C" int hwgat_dgcn_merge(const float* c, const float* mean, const float* rstd, const float* gamma, const float* beta,
                                const float* r, const float* res_mean, const float* res_rstd, const float* res_gamma,
                                const float* res_beta, const float* fs1, const float* ft1, const float* fs2,
                                const float* ft2, float* out, int N, int T, int V, int C, void* stream) {
    if (!c || !mean || !rstd || !gamma || !beta || !r || !fs1 || !ft1 || !fs2 || !ft2 || !out) return HWGAT_EINVAL;
    if (N <= 0 || T <= 0 || V <= 0 || C <= 0) return HWGAT_EINVAL;
    if (res_mean && (!res_rstd || !res_gamma || !res_beta)) return HWGAT_EINVAL;
    if (bad_shape(N, T, V, C)) return HWGAT_ESHAPE;
    const int64_t total = (int64_t)N * T * V * C;
    merge_k<<<grid1(total), 256, 0, (hipStream_t)stream>>>(c, mean, rstd, gamma, beta, r, res_mean, res_rstd, res_gamma,
                                                          res_beta, fs1, ft1, fs2, ft2, out, total, T, V, C);
    HWGAT_LAUNCH_CHECK();
}

extern "C" int hwgat_dgcn_merge_bwd(const float* dout, const float* out, const float* fs1, const float* ft1,
                                    const float* fs2, const float* ft2, float* dz1, float* dz2, int N, int T, int V, int C,
                                    void* stream) {
    if (!dout || !out || !fs1 || !ft1 || !fs2 || !ft2 || !dz1 || !dz2) return HWGAT_EINVAL;
    if (N <= 0 || T <= 0 || V <= 0 || C <= 0) return HWGAT_EINVAL;
    if (bad_shape(N, T, V, C)) return HWGAT_ESHAPE;
    const int64_t total = (int64_t)N * T * V * C;
    merge_bwd_k<<<grid1(total), 256, 0, (hipStream_t)stream>>>(dout, out, fs1, ft1, fs2, ft2, dz1, dz2, total, T, V, C);
    HWGAT_LAUNCH_CHECK();
}

extern "C" int hwgat_dgcn_masked_sum(const float* a, const float* ma, const float* b, const float* mb, float* out,
                                     int64_t n, void* stream) {
    if (!a || !b || !out || n <= 0) return HWGAT_EINVAL;
    if (n / 256 > 0x7fffffff) return HWGAT_ESHAPE;
    masked_sum_k<<<grid1(n), 256, 0, (hipStream_t)stream>>>(a, ma, b, mb, out, n);
    HWGAT_LAUNCH_CHECK();
}
