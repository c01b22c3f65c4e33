// LayerNorm forward / backward and the final LayerNorm + token mean-pool (reference hwgat/models/HWGATE.py:162,166,
// 203,219,327,353-354) for the row widths d = 64 n <= 1024 that the power-of-two kernels of layernorm.hip do not take
// (d = 64, 192, 320, 384, ... 960: HWGATE stages of embed_dim 64 / 192 and their doubles).  The C entry points of
// layernorm.hip dispatch here; semantics, dropout masks and the deterministic forms are the same.
//
// Row map: 16 lanes per row, 4 rows per wave pass, every lane holds n = d / 64 chunks of 4 consecutive values (chunk c
// of lane s = values 4 (16 c + s) .. +3), so each load / store instruction of a wave covers four 256-byte row segments
// (fp32).  Row sums are 16-lane butterflies: fixed order, no atomics within a row.
#include "common.h"
#include "fused_ops.h"
#include "layernorm_w64.h"

namespace {

constexpr float LN_EPS = 1e-5f;
constexpr int LPR = 16, RPW = 4;

typedef uint32_t u32x2w __attribute__((ext_vector_type(2)));
template <typename T, int CPL>
__device__ __forceinline__ void load_row(const T* row, int sub, float (&v)[CPL][4]) {
#pragma unroll
    for (int c = 0; c < CPL; ++c) {
        if constexpr (sizeof(T) == 4) {
            const f32x4 t = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(row + (c * LPR + sub) * 4));
            v[c][0] = t.x; v[c][1] = t.y; v[c][2] = t.z; v[c][3] = t.w;
        } else {
            const u32x2w t = __builtin_nontemporal_load(reinterpret_cast<const u32x2w*>(row + (c * LPR + sub) * 4));
            v[c][0] = __uint_as_float(t.x << 16); v[c][1] = __uint_as_float(t.x & 0xffff0000u);
            v[c][2] = __uint_as_float(t.y << 16); v[c][3] = __uint_as_float(t.y & 0xffff0000u);
        }
    }
}
template <typename T, int CPL>
__device__ __forceinline__ void store_row(T* row, int sub, const float (&v)[CPL][4]) {
#pragma unroll
    for (int c = 0; c < CPL; ++c) {
        if constexpr (sizeof(T) == 4) {
            const f32x4 t = {v[c][0], v[c][1], v[c][2], v[c][3]};
            __builtin_nontemporal_store(t, reinterpret_cast<f32x4*>(row + (c * LPR + sub) * 4));
        } else {
            const bf16x4 t = {(bf16_t)v[c][0], (bf16_t)v[c][1], (bf16_t)v[c][2], (bf16_t)v[c][3]};
            __builtin_nontemporal_store(__builtin_bit_cast(u32x2w, t), reinterpret_cast<u32x2w*>(row + (c * LPR + sub) * 4));
        }
    }
}
template <int CPL>
__device__ __forceinline__ void load_vec(const float* p, int sub, float (&v)[CPL][4]) {
#pragma unroll
    for (int c = 0; c < CPL; ++c) io<float>::load4(p + (c * LPR + sub) * 4, v[c]);
}
template <int CPL>
__device__ __forceinline__ void row_stats(const float (&v)[CPL][4], float& mean, float& rstd) {
    constexpr float inv_d = 1.0f / (64 * CPL);
    float s = 0.f;
#pragma unroll
    for (int c = 0; c < CPL; ++c)
#pragma unroll
        for (int e = 0; e < 4; ++e) s += v[c][e];
    mean = wave_sum<LPR>(s) * inv_d;
    float q = 0.f;
#pragma unroll
    for (int c = 0; c < CPL; ++c)
#pragma unroll
        for (int e = 0; e < 4; ++e) { const float t = v[c][e] - mean; q += t * t; }
    rstd = rsqrtf(wave_sum<LPR>(q) * inv_d + LN_EPS);
}
// sum of a per-lane column vector over the 4 row groups of a wave (lanes s, s + 16, s + 32, s + 48), fixed order
__device__ __forceinline__ float fold_rows(float v) {
    v += __shfl_xor(v, 16, 64);
    return v + __shfl_xor(v, 32, 64);
}

template <typename T, int CPL>
__global__ __launch_bounds__(256) void lnw_fwd_k(const T* __restrict__ x, const float* __restrict__ gamma,
                                                 const float* __restrict__ beta, T* __restrict__ y,
                                                 float* __restrict__ mean_o, float* __restrict__ rstd_o, int64_t N) {
    constexpr int D = 64 * CPL;
    const int lane = threadIdx.x & 63;
    const int sub = lane % LPR, rsub = lane / LPR;
    float g[CPL][4], b[CPL][4];
    load_vec<CPL>(gamma, sub, g);
    load_vec<CPL>(beta, sub, b);
    const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int64_t nwave = (int64_t)gridDim.x * 4;
    for (int64_t r0 = wave * RPW; r0 < N; r0 += nwave * RPW) {
        const int64_t r = r0 + rsub;
        if (r >= N) continue;
        float v[CPL][4];
        load_row<T, CPL>(x + r * D, sub, v);
        float mean, rstd;
        row_stats<CPL>(v, mean, rstd);
        if (y != nullptr) {                        // y == NULL: statistics only
#pragma unroll
            for (int c = 0; c < CPL; ++c)
#pragma unroll
                for (int e = 0; e < 4; ++e) v[c][e] = (v[c][e] - mean) * rstd * g[c][e] + b[c][e];
            store_row<T, CPL>(y + r * D, sub, v);
        }
        if (sub == 0) { mean_o[r] = mean; rstd_o[r] = rstd; }
    }
}

// backward (see ln_bwd_k in layernorm.hip): dx = rstd (g - mean(g) - xhat mean(g xhat)) (+ dres), g = dy gamma;
// dxm != NULL: also dx * dropout-keep(mseed, element index); xn != NULL: also xhat gamma + beta.
// DET: dgamma points at gridDim.x images of 2 D floats (block b stores its column sums into image b, no atomics).
template <typename T, int CPL, bool DET>
__global__ __launch_bounds__(256) void lnw_bwd_k(const T* __restrict__ dy, const T* __restrict__ x,
                                                 const float* __restrict__ mean_i, const float* __restrict__ rstd_i,
                                                 const float* __restrict__ gamma, const T* __restrict__ dres,
                                                 T* __restrict__ dx, float* __restrict__ dgamma, float* __restrict__ dbeta,
                                                 int64_t N, T* __restrict__ dxm, uint32_t mseed, float mp,
                                                 const float* __restrict__ beta, T* __restrict__ xn,
                                                 const uint32_t* __restrict__ sbase) {
    constexpr int D = 64 * CPL;
    if (dxm) mseed += seed_base_of(sbase);
    __shared__ float red[2][4][D];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int sub = lane % LPR, rsub = lane / LPR;
    float g[CPL][4], dg[CPL][4], db[CPL][4], bt[CPL][4];
    load_vec<CPL>(gamma, sub, g);
    if (xn) load_vec<CPL>(beta, sub, bt);
#pragma unroll
    for (int c = 0; c < CPL; ++c)
#pragma unroll
        for (int e = 0; e < 4; ++e) { dg[c][e] = 0.f; db[c][e] = 0.f; }
    const uint32_t th = drop_thresh(mp);
    const float sc = 1.0f / (1.0f - mp);
    const int64_t wave = (int64_t)blockIdx.x * 4 + wv;
    const int64_t nwave = (int64_t)gridDim.x * 4;
    for (int64_t r0 = wave * RPW; r0 < N; r0 += nwave * RPW) {
        const int64_t r = r0 + rsub;
        if (r >= N) continue;
        float xv[CPL][4], dv[CPL][4];
        load_row<T, CPL>(x + r * D, sub, xv);
        load_row<T, CPL>(dy + r * D, sub, dv);
        const float mean = mean_i[r], rstd = rstd_i[r];
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int c = 0; c < CPL; ++c)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float xh = (xv[c][e] - mean) * rstd;
                const float gg = dv[c][e] * g[c][e];
                dg[c][e] += dv[c][e] * xh;
                db[c][e] += dv[c][e];
                xv[c][e] = xh;
                dv[c][e] = gg;
                s1 += gg;
                s2 += gg * xh;
            }
        s1 = wave_sum<LPR>(s1) * (1.0f / D);
        s2 = wave_sum<LPR>(s2) * (1.0f / D);
        if (xn) {
            float nv[CPL][4];
#pragma unroll
            for (int c = 0; c < CPL; ++c)
#pragma unroll
                for (int e = 0; e < 4; ++e) nv[c][e] = xv[c][e] * g[c][e] + bt[c][e];
            store_row<T, CPL>(xn + r * D, sub, nv);
        }
        if (dres) {
            float rv[CPL][4];
            load_row<T, CPL>(dres + r * D, sub, rv);
#pragma unroll
            for (int c = 0; c < CPL; ++c)
#pragma unroll
                for (int e = 0; e < 4; ++e) dv[c][e] = rstd * (dv[c][e] - s1 - xv[c][e] * s2) + rv[c][e];
        } else {
#pragma unroll
            for (int c = 0; c < CPL; ++c)
#pragma unroll
                for (int e = 0; e < 4; ++e) dv[c][e] = rstd * (dv[c][e] - s1 - xv[c][e] * s2);
        }
        store_row<T, CPL>(dx + r * D, sub, dv);
        if (dxm) {
#pragma unroll
            for (int c = 0; c < CPL; ++c) {
                const f32x4 k = drop_keep4(mseed, (uint64_t)(r * D + (c * LPR + sub) * 4), th, sc);
                dv[c][0] *= k.x; dv[c][1] *= k.y; dv[c][2] *= k.z; dv[c][3] *= k.w;
            }
            store_row<T, CPL>(dxm + r * D, sub, dv);
        }
    }
#pragma unroll
    for (int c = 0; c < CPL; ++c)
#pragma unroll
        for (int e = 0; e < 4; ++e) { dg[c][e] = fold_rows(dg[c][e]); db[c][e] = fold_rows(db[c][e]); }
    if (rsub == 0) {
#pragma unroll
        for (int c = 0; c < CPL; ++c)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                red[0][wv][(c * LPR + sub) * 4 + e] = dg[c][e];
                red[1][wv][(c * LPR + sub) * 4 + e] = db[c][e];
            }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < D; i += 256) {
        const float sg = red[0][0][i] + red[0][1][i] + red[0][2][i] + red[0][3][i];
        const float sb = red[1][0][i] + red[1][1][i] + red[1][2][i] + red[1][3][i];
        if constexpr (DET) {
            dgamma[(int64_t)blockIdx.x * (2 * D) + i] = sg;
            dgamma[(int64_t)blockIdx.x * (2 * D) + D + i] = sb;
        } else {
            atomicAdd(dgamma + i, sg);
            atomicAdd(dbeta + i, sb);
        }
    }
}

// final LayerNorm + token sum per clip (see lnpool_fwd_k in layernorm.hip); partial != NULL: per-block sums stored
template <typename T, int CPL>
__global__ __launch_bounds__(256) void lnw_pool_fwd_k(const T* __restrict__ x, float* __restrict__ xhat_sum,
                                                      float* __restrict__ mean_o, float* __restrict__ rstd_o,
                                                      int n_tok, int chunks, float* __restrict__ partial) {
    constexpr int D = 64 * CPL;
    __shared__ float red[4][D];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int sub = lane % LPR, rsub = lane / LPR;
    const int b = blockIdx.x / chunks, ch = blockIdx.x % chunks;
    const int per = (n_tok + chunks - 1) / chunks;
    const int t0 = ch * per, t1 = min(n_tok, t0 + per);
    float acc[CPL][4];
#pragma unroll
    for (int c = 0; c < CPL; ++c)
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[c][e] = 0.f;
    for (int t = t0 + wv * RPW + rsub; t < t1; t += 4 * RPW) {
        const int64_t r = (int64_t)b * n_tok + t;
        float v[CPL][4];
        load_row<T, CPL>(x + r * D, sub, v);
        float mean, rstd;
        row_stats<CPL>(v, mean, rstd);
#pragma unroll
        for (int c = 0; c < CPL; ++c)
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[c][e] += (v[c][e] - mean) * rstd;
        if (sub == 0) { mean_o[r] = mean; rstd_o[r] = rstd; }
    }
#pragma unroll
    for (int c = 0; c < CPL; ++c)
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[c][e] = fold_rows(acc[c][e]);
    if (rsub == 0) {
#pragma unroll
        for (int c = 0; c < CPL; ++c)
#pragma unroll
            for (int e = 0; e < 4; ++e) red[wv][(c * LPR + sub) * 4 + e] = acc[c][e];
    }
    __syncthreads();
    for (int i = threadIdx.x; i < D; i += 256) {
        const float v = red[0][i] + red[1][i] + red[2][i] + red[3][i];
        if (partial) partial[(int64_t)blockIdx.x * D + i] = v;
        else atomicAdd(xhat_sum + (int64_t)b * D + i, v);
    }
}

template <typename T, int CPL>
__global__ __launch_bounds__(256) void lnw_pool_bwd_k(const float* __restrict__ g, const T* __restrict__ x,
                                                      const float* __restrict__ mean_i, const float* __restrict__ rstd_i,
                                                      T* __restrict__ dx, int n_tok, int chunks, T* __restrict__ dxm,
                                                      uint32_t mseed, float mp, const uint32_t* __restrict__ sbase) {
    constexpr int D = 64 * CPL;
    mseed += seed_base_of(sbase);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int sub = lane % LPR, rsub = lane / LPR;
    const int b = blockIdx.x / chunks, ch = blockIdx.x % chunks;
    const int per = (n_tok + chunks - 1) / chunks;
    const int t0 = ch * per, t1 = min(n_tok, t0 + per);
    float gv[CPL][4];
    load_vec<CPL>(g + (int64_t)b * D, sub, gv);
    float s1 = 0.f;
#pragma unroll
    for (int c = 0; c < CPL; ++c)
#pragma unroll
        for (int e = 0; e < 4; ++e) s1 += gv[c][e];
    s1 = wave_sum<LPR>(s1) * (1.0f / D);
    const uint32_t th = drop_thresh(mp);
    const float sc = 1.0f / (1.0f - mp);
    for (int t = t0 + wv * RPW + rsub; t < t1; t += 4 * RPW) {
        const int64_t r = (int64_t)b * n_tok + t;
        float v[CPL][4];
        load_row<T, CPL>(x + r * D, sub, v);
        const float mean = mean_i[r], rstd = rstd_i[r];
        float s2 = 0.f;
#pragma unroll
        for (int c = 0; c < CPL; ++c)
#pragma unroll
            for (int e = 0; e < 4; ++e) { v[c][e] = (v[c][e] - mean) * rstd; s2 += gv[c][e] * v[c][e]; }
        s2 = wave_sum<LPR>(s2) * (1.0f / D);
#pragma unroll
        for (int c = 0; c < CPL; ++c)
#pragma unroll
            for (int e = 0; e < 4; ++e) v[c][e] = rstd * (gv[c][e] - s1 - v[c][e] * s2);
        store_row<T, CPL>(dx + r * D, sub, v);
        if (dxm != nullptr) {
#pragma unroll
            for (int c = 0; c < CPL; ++c) {
                const f32x4 k = drop_keep4(mseed, (uint64_t)(r * D + (c * LPR + sub) * 4), th, sc);
                v[c][0] *= k.x; v[c][1] *= k.y; v[c][2] *= k.z; v[c][3] *= k.w;
            }
            store_row<T, CPL>(dxm + r * D, sub, v);
        }
    }
}

inline int lnw_grid(int64_t N) {
    const int64_t need = (N + 4 * RPW - 1) / (4 * RPW);
    return (int)(need < 2048 ? (need < 1 ? 1 : need) : 2048);
}

// f(LnElem<T>, std::integral_constant<int, d / 64>): the dtype first, then the widths this file serves (every multiple of
// 64 up to 1024 but 128, 256, 512, 1024)
template <typename F> int with_kernel(int dtype, int d, F&& f) {
    return ln_with_dtype(dtype, [&](auto elem) {
        if (!hwgat_lnw_takes(d)) return (int)HWGAT_ESHAPE;
        return ln_with_int<1, 3, 5, 6, 7, 9, 10, 11, 12, 13, 14, 15>(d / 64, [&](auto n) { return f(elem, n); });
    });
}

}  // namespace

bool hwgat_lnw_takes(int d) {
    return d > 0 && d % 64 == 0 && d <= 1024 && d != 128 && d != 256 && d != 512 && d != 1024;
}

int hwgat_lnw_fwd(const void* x, const float* gm, const float* bt, void* y, float* mean, float* rstd, int64_t N, int d,
                  int dtype, hipStream_t st) {
    const int rc = with_kernel(dtype, d, [&](auto elem, auto n) {
        using T = typename decltype(elem)::type;
        lnw_fwd_k<T, n()><<<lnw_grid(N), 256, 0, st>>>((const T*)x, gm, bt, (T*)y, mean, rstd, N);
        return 0;
    });
    if (rc) return rc;
    HWGAT_LAUNCH_CHECK();
}

int hwgat_lnw_bwd(const LnBwdArgs& a, hipStream_t st) {
    const int grid = lnw_grid(a.N) < 1024 ? lnw_grid(a.N) : 1024;
    const int rc = with_kernel(a.dtype, a.d, [&](auto elem, auto n) {
        using T = typename decltype(elem)::type;
        constexpr int CPL = n();
        return ln_with_bool(a.det(), [&](auto det) {
            lnw_bwd_k<T, CPL, det()><<<grid, 256, 0, st>>>(
                (const T*)a.dy, (const T*)a.x, a.mean, a.rstd, a.gamma, (const T*)a.dres, (T*)a.dx,
                det() ? a.det_ws : a.dgamma, det() ? a.det_ws : a.dbeta, a.N, (T*)a.dx_masked, a.mask_seed, a.mask_p,
                a.beta, (T*)a.xn, a.seed_base);
            return 0;
        });
    });
    return rc ? rc : ln_bwd_finish(a, grid, st);
}

int hwgat_lnw_pool_fwd(const LnPoolArgs& a, hipStream_t st) {
    const int rc = with_kernel(a.dtype, a.d, [&](auto elem, auto n) {
        using T = typename decltype(elem)::type;
        lnw_pool_fwd_k<T, n()><<<a.B * a.chunks, 256, 0, st>>>((const T*)a.x, a.xhat_sum, a.mean, a.rstd, a.n_tok, a.chunks,
                                                              a.partial);
        return 0;
    });
    if (rc) return rc;
    HWGAT_LAUNCH_CHECK();
}

int hwgat_lnw_pool_bwd(const LnPoolArgs& a, hipStream_t st) {
    const int rc = with_kernel(a.dtype, a.d, [&](auto elem, auto n) {
        using T = typename decltype(elem)::type;
        lnw_pool_bwd_k<T, n()><<<a.B * a.chunks, 256, 0, st>>>(a.g, (const T*)a.x, a.mean, a.rstd, (T*)a.dx, a.n_tok, a.chunks,
                                                              (T*)a.dx_masked, a.mask_seed, a.mask_p, a.seed_base);
        return 0;
    });
    if (rc) return rc;
    HWGAT_LAUNCH_CHECK();
}

