// Frame embedding and max pool of the Transformer baseline (reference hwgat/models/Transformer.py: forward, make_src_mask,
// PositionalEncoding, torch.max pool).
//
// hwgat_seq_embed_fwd: out[b,t,:] = drop((x[b,t,:] W^T + bias) * sqrt(d) + pe[t,:]) in the activation dtype, and the
//   key-padding words pad[b][t / 32] bit t % 32 = (x[b,t,0] == pad_index), in one launch.  x (B, T, F) fp32, F any
//   width (58, 87, ...: not a multiple of 64, so the MFMA linears cannot take it), Wt = W^T (F, d) fp32, pe (T, d).
// hwgat_seq_embed_bwd: dW[n,f] = sum_m g[m,n] x[m,f], db[n] = sum_m g[m,n] with g = dout * mask * sqrt(d): per-split
//   images of 64 columns x all F over a fixed row range each, then added in split order -- no atomics, bit-reproducible.
// hwgat_seq_maxpool_fwd / _bwd: max over T of (B, T, d) -> (B, d) fp32 with the first index of the maximum (as
//   torch.max: a NaN is the maximum, at the first NaN's index), and its backward (the gradient lands on that index only).
#include "common.h"
#include "fused_ops.h"

namespace {

constexpr int ROWS = 16;          // frames per block of the forward
constexpr int MAX_F = 512;

template <typename T>
__global__ __launch_bounds__(256) void seq_embed_fwd_k(const float* __restrict__ x, const float* __restrict__ Wt,
                                                        const float* __restrict__ bias, const float* __restrict__ pe,
                                                        T* __restrict__ out, uint32_t* __restrict__ pad, int B, int Tn,
                                                        int F, int d, float pad_index, float scale, uint32_t seed,
                                                        float p, const uint32_t* seed_base) {
    __shared__ float xs[ROWS][MAX_F];
    const int64_t M = (int64_t)B * Tn;
    const int64_t m0 = (int64_t)blockIdx.x * ROWS;
    // key-padding words: global thread g < B * nw builds word g from the first feature of its 32 frames
    const int nw = (Tn + 31) / 32;
    const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (g < (int64_t)B * nw) {
        const int b = (int)(g / nw), w = (int)(g % nw);
        uint32_t bits = 0;
        for (int t = w * 32; t < min(Tn, w * 32 + 32); ++t)
            if (x[((int64_t)b * Tn + t) * F] == pad_index) bits |= 1u << (t - w * 32);
        pad[g] = bits;
    }
    if (m0 >= M) return;
    for (int q = threadIdx.x; q < ROWS * F; q += 256) {
        const int r = q / F, f = q % F;
        xs[r][f] = m0 + r < M ? x[(m0 + r) * F + f] : 0.f;
    }
    __syncthreads();
    const uint32_t sd = seed + seed_base_of(seed_base);
    const uint32_t th = drop_thresh(p);
    const float dsc = 1.0f / (1.0f - p);
    for (int n = threadIdx.x; n < d; n += 256) {
        float acc[ROWS];
#pragma unroll
        for (int r = 0; r < ROWS; ++r) acc[r] = 0.f;
        for (int f = 0; f < F; ++f) {
            const float w = Wt[(int64_t)f * d + n];
#pragma unroll
            for (int r = 0; r < ROWS; ++r) acc[r] = fmaf(xs[r][f], w, acc[r]);
        }
        const float bn = bias ? bias[n] : 0.f;
#pragma unroll
        for (int r = 0; r < ROWS; ++r) {
            const int64_t m = m0 + r;
            if (m >= M) break;
            const int t = (int)(m % Tn);
            float v = (acc[r] + bn) * scale + (pe ? pe[(int64_t)t * d + n] : 0.f);
            if (th) v *= drop_keep(sd, (uint64_t)(m * d + n), th, dsc);
            io<T>::st(out + m * d + n, v);
        }
    }
}

constexpr int BWD_COLS = 64;
constexpr int BWD_SPLITS = 64;

// one block = 64 columns x split s: rows [s * chunk, (s + 1) * chunk); 256 threads = 64 columns x 4 feature phases
template <typename T>
__global__ __launch_bounds__(256) void seq_embed_bwd_k(const T* __restrict__ dout, const float* __restrict__ x,
                                                        float* __restrict__ ws, int64_t M, int F, int d, float scale,
                                                        uint32_t seed, float p, const uint32_t* seed_base, int64_t chunk) {
    __shared__ float gs[32][BWD_COLS + 1];
    __shared__ float xs[32][MAX_F / 4 + 1];
    const int n0 = blockIdx.x * BWD_COLS, s = blockIdx.y;
    const int cl = threadIdx.x % BWD_COLS, ph = threadIdx.x / BWD_COLS;
    const int64_t r_begin = (int64_t)s * chunk, r_end = min(M, r_begin + chunk);
    const uint32_t sd = seed + seed_base_of(seed_base);
    const uint32_t th = drop_thresh(p);
    const float dsc = 1.0f / (1.0f - p);
    // F in pieces of MAX_F / 4 features (the LDS stage); each thread owns features ph, ph + 4, ... of the piece
    for (int f0 = 0; f0 < F; f0 += MAX_F / 4) {
        const int nf = min(MAX_F / 4, F - f0);
        float acc[MAX_F / 16];
        float db = 0.f;
#pragma unroll
        for (int e = 0; e < MAX_F / 16; ++e) acc[e] = 0.f;
        for (int64_t m0 = r_begin; m0 < r_end; m0 += 32) {
            __syncthreads();
            for (int q = threadIdx.x; q < 32 * BWD_COLS; q += 256) {
                const int r = q / BWD_COLS, c = q % BWD_COLS;
                const int64_t m = m0 + r;
                float v = 0.f;
                if (m < r_end && n0 + c < d) {
                    v = io<T>::ld(dout + m * d + n0 + c) * scale;
                    if (th) v *= drop_keep(sd, (uint64_t)(m * d + n0 + c), th, dsc);
                }
                gs[r][c] = v;
            }
            for (int q = threadIdx.x; q < 32 * nf; q += 256) {
                const int r = q / nf, f = q % nf;
                const int64_t m = m0 + r;
                xs[r][f] = m < r_end ? x[m * F + f0 + f] : 0.f;
            }
            __syncthreads();
            for (int r = 0; r < 32; ++r) {
                const float gv = gs[r][cl];
                if (ph == 0 && f0 == 0) db += gv;
#pragma unroll
                for (int e = 0; e < MAX_F / 16; ++e)
                    if (ph + 4 * e < nf) acc[e] = fmaf(gv, xs[r][ph + 4 * e], acc[e]);
            }
        }
        if (n0 + cl < d) {
            float* img = ws + (int64_t)s * ((int64_t)d * F + d);
#pragma unroll
            for (int e = 0; e < MAX_F / 16; ++e)
                if (ph + 4 * e < nf) img[(int64_t)(n0 + cl) * F + f0 + ph + 4 * e] = acc[e];
            if (ph == 0 && f0 == 0) img[(int64_t)d * F + n0 + cl] = db;
        }
    }
}

// dW (d F) and db (d) += sum over the splits in ascending order
__global__ __launch_bounds__(256) void seq_embed_bwd_reduce_k(const float* __restrict__ ws, float* __restrict__ dW,
                                                               float* __restrict__ db, int64_t dF, int d, int splits) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= dF + d) return;
    float s = 0.f;
    for (int k = 0; k < splits; ++k) s += ws[(int64_t)k * (dF + d) + i];
    if (i < dF) dW[i] += s;
    else if (db) db[i - dF] += s;
}

template <typename T>
__global__ __launch_bounds__(256) void seq_maxpool_fwd_k(const T* __restrict__ x, float* __restrict__ out,
                                                          int32_t* __restrict__ idx, int B, int Tn, int d) {
    const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (g >= (int64_t)B * d) return;
    const int b = (int)(g / d), n = (int)(g % d);
    const T* src = x + (int64_t)b * Tn * d + n;
    float best = io<T>::ld(src);
    int bi = 0;
    for (int t = 1; t < Tn; ++t) {
        const float v = io<T>::ld(src + (int64_t)t * d);
        // a NaN wins over every number and the first NaN keeps its place, as in torch.max
        if (v > best || (v != v && best == best)) { best = v; bi = t; }
    }
    out[g] = best;
    idx[g] = bi;
}

template <typename T>
__global__ __launch_bounds__(256) void seq_maxpool_bwd_k(const float* __restrict__ dout, const int32_t* __restrict__ idx,
                                                          T* __restrict__ dx, int B, int Tn, int d) {
    const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (g >= (int64_t)B * Tn * d) return;
    const int n = (int)(g % d);
    const int64_t bt = g / d;
    const int b = (int)(bt / Tn), t = (int)(bt % Tn);
    const int64_t o = (int64_t)b * d + n;
    io<T>::st(dx + g, idx[o] == t ? dout[o] : 0.f);
}

}  // namespace

extern "C" int hwgat_seq_embed_fwd(const float* x, const float* Wt, const float* bias, const float* pe, void* out,
                                   uint32_t* pad, int B, int T, int F, int d, float pad_index, int dtype, uint32_t seed,
                                   float p, const uint32_t* seed_base, void* stream) {
    if (!x || !Wt || !out || !pad || B <= 0 || T <= 0 || F <= 0 || d <= 0) return HWGAT_EINVAL;
    if (F > MAX_F) return HWGAT_ESHAPE;
    if (p < 0.f || p >= 1.f) return HWGAT_EINVAL;
    const int64_t M = (int64_t)B * T;
    const int64_t words = (int64_t)B * ((T + 31) / 32);
    int64_t grid = (M + ROWS - 1) / ROWS;
    if (grid * 256 < words) grid = (words + 255) / 256;
    if (grid > 0x7fffffff) return HWGAT_ESHAPE;
    const float scale = sqrtf((float)d);
    hipStream_t st = (hipStream_t)stream;
    if (dtype == HWGAT_F32)
        seq_embed_fwd_k<float><<<(int)grid, 256, 0, st>>>(x, Wt, bias, pe, (float*)out, pad, B, T, F, d, pad_index, scale,
                                                          seed, p, seed_base);
    else if (dtype == HWGAT_BF16)
        seq_embed_fwd_k<bf16_t><<<(int)grid, 256, 0, st>>>(x, Wt, bias, pe, (bf16_t*)out, pad, B, T, F, d, pad_index,
                                                           scale, seed, p, seed_base);
    else return HWGAT_EDTYPE;
    HWGAT_LAUNCH_CHECK();
}

extern "C" int64_t hwgat_seq_embed_bwd_bytes(int F, int d) {
    if (F <= 0 || d <= 0 || F > MAX_F) return -1;
    return (int64_t)BWD_SPLITS * ((int64_t)d * F + d) * 4;
}

extern "C" int hwgat_seq_embed_bwd(const void* dout, const float* x, float* dW, float* db, int64_t M, int F, int d,
                                   int dtype, uint32_t seed, float p, const uint32_t* seed_base, float* ws,
                                   int64_t ws_bytes, void* stream) {
    if (!dout || !x || !dW || !ws || M <= 0 || F <= 0 || d <= 0) return HWGAT_EINVAL;
    if (F > MAX_F) return HWGAT_ESHAPE;
    if (ws_bytes < hwgat_seq_embed_bwd_bytes(F, d) || p < 0.f || p >= 1.f) return HWGAT_EINVAL;
    const int64_t chunk = ((M + BWD_SPLITS - 1) / BWD_SPLITS + 31) / 32 * 32;
    const int splits = (int)((M + chunk - 1) / chunk);
    const dim3 grid((d + BWD_COLS - 1) / BWD_COLS, splits);
    const float scale = sqrtf((float)d);
    hipStream_t st = (hipStream_t)stream;
    if (dtype == HWGAT_F32)
        seq_embed_bwd_k<float><<<grid, 256, 0, st>>>((const float*)dout, x, ws, M, F, d, scale, seed, p, seed_base, chunk);
    else if (dtype == HWGAT_BF16)
        seq_embed_bwd_k<bf16_t><<<grid, 256, 0, st>>>((const bf16_t*)dout, x, ws, M, F, d, scale, seed, p, seed_base, chunk);
    else return HWGAT_EDTYPE;
    const int64_t n = (int64_t)d * F + d;
    seq_embed_bwd_reduce_k<<<(int)((n + 255) / 256), 256, 0, st>>>(ws, dW, db, (int64_t)d * F, d, splits);
    HWGAT_LAUNCH_CHECK();
}

extern "C" int hwgat_seq_maxpool_fwd(const void* x, float* out, int32_t* idx, int B, int T, int d, int dtype, void* stream) {
    if (!x || !out || !idx || B <= 0 || T <= 0 || d <= 0) return HWGAT_EINVAL;
    const int grid = (int)(((int64_t)B * d + 255) / 256);
    hipStream_t st = (hipStream_t)stream;
    if (dtype == HWGAT_F32) seq_maxpool_fwd_k<float><<<grid, 256, 0, st>>>((const float*)x, out, idx, B, T, d);
    else if (dtype == HWGAT_BF16) seq_maxpool_fwd_k<bf16_t><<<grid, 256, 0, st>>>((const bf16_t*)x, out, idx, B, T, d);
    else return HWGAT_EDTYPE;
    HWGAT_LAUNCH_CHECK();
}

extern "C" int hwgat_seq_maxpool_bwd(const float* dout, const int32_t* idx, void* dx, int B, int T, int d, int dtype,
                                     void* stream) {
    if (!dout || !idx || !dx || B <= 0 || T <= 0 || d <= 0) return HWGAT_EINVAL;
    const int64_t n = (int64_t)B * T * d;
    if ((n + 255) / 256 > 0x7fffffff) return HWGAT_ESHAPE;
    const int grid = (int)((n + 255) / 256);
    hipStream_t st = (hipStream_t)stream;
    if (dtype == HWGAT_F32) seq_maxpool_bwd_k<float><<<grid, 256, 0, st>>>(dout, idx, (float*)dx, B, T, d);
    else if (dtype == HWGAT_BF16) seq_maxpool_bwd_k<bf16_t><<<grid, 256, 0, st>>>(dout, idx, (bf16_t*)dx, B, T, d);
    else return HWGAT_EDTYPE;
    HWGAT_LAUNCH_CHECK();
}
