// Convolutions of the ST-GCN baseline (reference hwgat/models/STGCN.py) on channels-last activations (N, T, V, C):
// every convolution of the model -- the 9x1 temporal one, the 1x1 graph-conv projection, the strided 1x1 residual -- is
// the same implicit GEMM over rows m = (n, t, v) with a reduction over taps x C_in, tap k reading the input row of
// frame  stride * t + k - pad  of the same clip and joint (zero outside the clip).  No im2col buffer exists anywhere.
//
// hwgat_stgcn_weight_prep  master weight (C_out, C_in, taps, 1) -> the k-major image a kernel reads:
//                          mode 0 [tap][c_in (padded to CinP, zero rows)][c_out], mode 1 [tap][c_out][c_in (padded)]
// hwgat_stgcn_conv         mode 0: the convolution.  mode 1: its input gradient (the transposed convolution: output frame
//                          t takes tap k from gradient frame (t + pad - k) / stride where that is a whole number) with
//                          the mode-1 weight image.  Epilogue: + bias[col], + add[m][col] (optionally gated by
//                          mask[m][col] > 0: the identity residual's gradient behind the block's last ReLU).
//                          128 x 64 output tile per block, 4 waves x (32 x 64), v_mfma_f32_32x32x2_f32, K slabs of 32.
// hwgat_stgcn_conv_dw      weight gradient dW[c_out][c_in][tap] = sum_m dy[m][c_out] in[src(m, tap)][c_in]: 64 x 64
//                          tiles per (tap, row split) into per-split images, added in split order by a second kernel
//                          that writes the master layout -- no atomics, bit-reproducible.
#include "common.h"

namespace {

constexpr int BM = 128, BN = 64, KC = 32, LDA = KC + 1;
constexpr int MAX_SPLITS = 64;

struct ConvP {
    const float* in; const float* wk; const float* bias; const float* add; const float* mask; float* out;
    int Tin, Tout, V, Cin, Cout, taps, stride, pad, mode;
    int64_t M;
};

// frame of the input tensor that tap `tap` of output frame `to` reads, or -1
__device__ __forceinline__ int src_frame(int to, int tap, int stride, int pad, int Tin, int mode) {
    if (mode == 0) {
        const int ti = stride * to + tap - pad;
        return (ti >= 0 && ti < Tin) ? ti : -1;
    }
    const int q = to + pad - tap;
    if (q < 0 || q % stride) return -1;
    const int ti = q / stride;
    return ti < Tin ? ti : -1;
}

__global__ __launch_bounds__(256) void conv_k(ConvP p) {
    __shared__ float As[BM * LDA];
    __shared__ float Bs[KC * BN];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int64_t m0 = (int64_t)blockIdx.x * BM;
    const int n0 = blockIdx.y * BN;
    const int lr = tid >> 3, lc = (tid & 7) * 4;
    int64_t rbase[4];
    int rto[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int64_t m = m0 + lr + 32 * q;
        rto[q] = -1;
        rbase[q] = 0;
        if (m < p.M) {
            const int v = (int)(m % p.V);
            const int64_t nt = m / p.V;
            rto[q] = (int)(nt % p.Tout);
            rbase[q] = (nt / p.Tout) * p.Tin * p.V + v;
        }
    }
    f32x16 acc[2];
#pragma unroll
    for (int r = 0; r < 16; ++r) { acc[0][r] = 0.f; acc[1][r] = 0.f; }
    const int bk = tid >> 4, bn = (tid & 15) * 4;
    for (int tap = 0; tap < p.taps; ++tap) {
        int64_t srow[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int ti = rto[q] >= 0 ? src_frame(rto[q], tap, p.stride, p.pad, p.Tin, p.mode) : -1;
            srow[q] = ti >= 0 ? rbase[q] + (int64_t)ti * p.V : -1;
        }
        for (int k0 = 0; k0 < p.Cin; k0 += KC) {
            __syncthreads();
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                f32x4 v = {0.f, 0.f, 0.f, 0.f};
                if (srow[q] >= 0) v = *reinterpret_cast<const f32x4*>(p.in + srow[q] * p.Cin + k0 + lc);
                float* dst = As + (lr + 32 * q) * LDA + lc;
                dst[0] = v.x; dst[1] = v.y; dst[2] = v.z; dst[3] = v.w;
            }
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                const int kk = bk + 16 * q;
                f32x4 w = {0.f, 0.f, 0.f, 0.f};
                if (n0 + bn < p.Cout)
                    w = *reinterpret_cast<const f32x4*>(p.wk + ((int64_t)tap * p.Cin + k0 + kk) * p.Cout + n0 + bn);
                *reinterpret_cast<f32x4*>(Bs + kk * BN + bn) = w;
            }
            __syncthreads();
            const float* ap = As + (32 * wave + (lane & 31)) * LDA + (lane >> 5);
            const float* bp = Bs + (lane >> 5) * BN + (lane & 31);
#pragma unroll
            for (int j = 0; j < KC / 2; ++j) {
                const float a = ap[2 * j];
                const float b0 = bp[2 * j * BN], b1 = bp[2 * j * BN + 32];
                acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b0, acc[0], 0, 0, 0);
                acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b1, acc[1], 0, 0, 0);
            }
        }
    }
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {
        const int col = n0 + nt * 32 + (lane & 31);
        if (col >= p.Cout) continue;
        const float bv = p.bias ? p.bias[col] : 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int64_t m = m0 + 32 * wave + crow(r, lane >> 5);
            if (m >= p.M) continue;
            const int64_t i = m * p.Cout + col;
            float v = acc[nt][r] + bv;
            if (p.add) {
                float a = p.add[i];
                if (p.mask && !(p.mask[i] > 0.f)) a = 0.f;
                v += a;
            }
            p.out[i] = v;
        }
    }
}

struct DwP {
    const float* in; const float* dy; float* ws;
    int Tin, Tout, V, CinP, Cout, taps, stride, pad;
    int64_t M, chunk;
};

__global__ __launch_bounds__(256) void conv_dw_k(DwP p) {
    __shared__ float Xs[32 * 64];
    __shared__ float Gs[32 * 64];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int ci0 = blockIdx.x * 64, co0 = blockIdx.y * 64;
    const int tap = blockIdx.z % p.taps, s = blockIdx.z / p.taps;
    const int64_t r_begin = (int64_t)s * p.chunk, r_end = min(p.M, r_begin + p.chunk);
    const int cit = wave >> 1, cot = wave & 1;
    const int lrow = tid >> 4, c4 = (tid & 15) * 4;
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    for (int64_t mm = r_begin; mm < r_end; mm += 32) {
        __syncthreads();
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int row = lrow + 16 * q;
            const int64_t m = mm + row;
            f32x4 g = {0.f, 0.f, 0.f, 0.f}, x = {0.f, 0.f, 0.f, 0.f};
            if (m < r_end) {
                if (co0 + c4 < p.Cout) g = *reinterpret_cast<const f32x4*>(p.dy + m * p.Cout + co0 + c4);
                const int v = (int)(m % p.V);
                const int64_t nt = m / p.V;
                const int ti = src_frame((int)(nt % p.Tout), tap, p.stride, p.pad, p.Tin, 0);
                if (ti >= 0 && ci0 + c4 < p.CinP)
                    x = *reinterpret_cast<const f32x4*>(p.in + (((nt / p.Tout) * p.Tin + ti) * p.V + v) * p.CinP + ci0 + c4);
            }
            *reinterpret_cast<f32x4*>(Xs + row * 64 + c4) = x;
            *reinterpret_cast<f32x4*>(Gs + row * 64 + c4) = g;
        }
        __syncthreads();
        const float* ap = Xs + (lane >> 5) * 64 + cit * 32 + (lane & 31);
        const float* bp = Gs + (lane >> 5) * 64 + cot * 32 + (lane & 31);
#pragma unroll
        for (int j = 0; j < 16; ++j)
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ap[2 * j * 64], bp[2 * j * 64], acc, 0, 0, 0);
    }
    const int co = co0 + cot * 32 + (lane & 31);
    if (co >= p.Cout) return;
    float* img = p.ws + ((int64_t)s * p.taps + tap) * p.CinP * p.Cout;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int ci = ci0 + cit * 32 + crow(r, lane >> 5);
        if (ci < p.CinP) img[(int64_t)ci * p.Cout + co] = acc[r];
    }
}

// dW (C_out, C_in, taps) = sum over the splits, ascending
__global__ __launch_bounds__(256) void conv_dw_reduce_k(const float* __restrict__ ws, float* __restrict__ dW, int S, int taps,
                                                         int CinP, int Cin, int Cout) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)Cout * Cin * taps) return;
    const int tap = (int)(i % taps), ci = (int)((i / taps) % Cin), co = (int)(i / ((int64_t)taps * Cin));
    float sum = 0.f;
    for (int s = 0; s < S; ++s) sum += ws[(((int64_t)s * taps + tap) * CinP + ci) * Cout + co];
    dW[i] = sum;
}

__global__ __launch_bounds__(256) void wprep_k(const float* __restrict__ W, float* __restrict__ out, int Cout, int Cin,
                                                int taps, int CinP, int mode) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)taps * CinP * Cout) return;
    int tap, ci, co;
    if (mode == 0) { co = (int)(i % Cout); ci = (int)((i / Cout) % CinP); tap = (int)(i / ((int64_t)Cout * CinP)); }
    else { ci = (int)(i % CinP); co = (int)((i / CinP) % Cout); tap = (int)(i / ((int64_t)Cout * CinP)); }
    out[i] = ci < Cin ? W[((int64_t)co * Cin + ci) * taps + tap] : 0.f;
}

void dw_splits(int64_t M, int CinP, int Cout, int taps, int* S, int64_t* chunk) {
    const int64_t tiles = (int64_t)((CinP + 63) / 64) * ((Cout + 63) / 64) * taps;
    int64_t s = 2048 / tiles;
    if (s > MAX_SPLITS) s = MAX_SPLITS;
    if (s > (M + 31) / 32) s = (M + 31) / 32;
    if (s < 1) s = 1;
    *chunk = ((M + s - 1) / s + 31) / 32 * 32;
    *S = (int)((M + *chunk - 1) / *chunk);
}

bool conv_shape_ok(int Tin, int Tout, int V, int Cin, int Cout, int taps, int stride, int pad) {
    return Tin > 0 && Tout > 0 && V > 0 && Cin > 0 && Cout > 0 && Cin % 32 == 0 && Cout % 32 == 0 && taps >= 1 &&
           taps <= 9 && stride >= 1 && stride <= 2 && pad >= 0 && pad < taps;
}

}  // namespace

extern "C" int hwgat_stgcn_weight_prep(const float* W, float* out, int Cout, int Cin, int taps, int CinP, int mode,
                                       void* stream) {
    if (!W || !out || Cout <= 0 || Cin <= 0 || taps <= 0 || CinP < Cin) return HWGAT_EINVAL;
    if (mode != 0 && mode != 1) return HWGAT_EINVAL;
    const int64_t n = (int64_t)taps * CinP * Cout;
    wprep_k<<<(int)((n + 255) / 256), 256, 0, (hipStream_t)stream>>>(W, out, Cout, Cin, taps, CinP, mode);
    HWGAT_LAUNCH_CHECK();
}

extern "C" int hwgat_stgcn_conv(const float* in, const float* wk, const float* bias, const float* add, const float* mask,
                                float* out, int Nc, int Tin, int Tout, int V, int Cin, int Cout, int taps, int stride,
                                int pad, int mode, void* stream) {
    if (!in || !wk || !out || Nc <= 0 || (mask && !add)) return HWGAT_EINVAL;
    if (mode != 0 && mode != 1) return HWGAT_EINVAL;
    if (!conv_shape_ok(Tin, Tout, V, Cin, Cout, taps, stride, pad)) return HWGAT_ESHAPE;
    // the frame counts must belong to one convolution: forward T_out = (T_in + 2 pad - taps) / stride + 1, mode 1 the
    // other way round (T_in is then the gradient's frame count)
    const int Tx = mode == 0 ? Tin : Tout, Ty = mode == 0 ? Tout : Tin;
    if (Tx + 2 * pad < taps || (Tx + 2 * pad - taps) / stride + 1 != Ty) return HWGAT_ESHAPE;
    ConvP p{in, wk, bias, add, mask, out, Tin, Tout, V, Cin, Cout, taps, stride, pad, mode, (int64_t)Nc * Tout * V};
    const int64_t gx = (p.M + BM - 1) / BM;
    if (gx > 0x7fffffff) return HWGAT_ESHAPE;
    conv_k<<<dim3((unsigned)gx, (Cout + BN - 1) / BN), 256, 0, (hipStream_t)stream>>>(p);
    HWGAT_LAUNCH_CHECK();
}

extern "C" int64_t hwgat_stgcn_conv_dw_bytes(int64_t M, int CinP, int Cout, int taps) {
    if (M <= 0 || CinP <= 0 || Cout <= 0 || taps <= 0 || CinP % 32 || Cout % 32) return -1;
    int S;
    int64_t chunk;
    dw_splits(M, CinP, Cout, taps, &S, &chunk);
    return (int64_t)S * taps * CinP * Cout * 4;
}

extern "C" int hwgat_stgcn_conv_dw(const float* in, const float* dy, float* dW, int Nc, int Tin, int Tout, int V, int CinP,
                                   int Cin, int Cout, int taps, int stride, int pad, float* ws, int64_t ws_bytes,
                                   void* stream) {
    if (!in || !dy || !dW || !ws || Nc <= 0 || Cin <= 0 || Cin > CinP) return HWGAT_EINVAL;
    if (!conv_shape_ok(Tin, Tout, V, CinP, Cout, taps, stride, pad)) return HWGAT_ESHAPE;
    if (Tin + 2 * pad < taps || (Tin + 2 * pad - taps) / stride + 1 != Tout) return HWGAT_ESHAPE;
    const int64_t M = (int64_t)Nc * Tout * V;
    if (ws_bytes < hwgat_stgcn_conv_dw_bytes(M, CinP, Cout, taps)) return HWGAT_EINVAL;
    int S;
    int64_t chunk;
    dw_splits(M, CinP, Cout, taps, &S, &chunk);
    DwP p{in, dy, ws, Tin, Tout, V, CinP, Cout, taps, stride, pad, M, chunk};
    hipStream_t st = (hipStream_t)stream;
    conv_dw_k<<<dim3((CinP + 63) / 64, (Cout + 63) / 64, S * taps), 256, 0, st>>>(p);
    const int64_t n = (int64_t)Cout * Cin * taps;
    conv_dw_reduce_k<<<(int)((n + 255) / 256), 256, 0, st>>>(ws, dW, S, taps, CinP, Cin, Cout);
    HWGAT_LAUNCH_CHECK();
}
