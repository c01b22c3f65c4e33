// The classifier head on gfx950: Y = X W^T + bias and its two gradients for a skinny product (M = the batch, 1 .. a few
// hundred rows; N = the class count, any value up to 65536; K = the feature width, a multiple of 64 up to 1024).  The
// block linears (gemm_f32*.hip) need N % 64 == 0 and work on 128/256-row tiles; this product is bound by launch
// latency and by one read of W, so it gets three small kernels of its own.
//
// Reference: the `head` / `classifier` nn.Linear of every model (hwgat/models/HWGATE.py:331,372).
//
// All three run on v_mfma_f32_16x16x4_f32: exact fp32, bit for bit a fused-multiply-add chain in the order of the
// instruction's k index.  Lane l = 16 g + c supplies A[row c][k g] and B[k g][column c]; register r of the result is
// D[row 4 g + r][column c].  Operands come straight from global memory.  Where the reduction index is contiguous in
// memory (the forward: K) a lane loads 16 bytes, four consecutive k, and feeds them to four MFMAs, so the reduction
// walks k in a permuted order that is the same for both operands and for every call.  Where the OUTPUT index is
// contiguous (dX, dW: K) the 16-byte load feeds four accumulators, columns 4 c + j of a 64-column tile.
//
// Summation order.  Every output element is one fixed chain of fused multiply-adds, or a fixed number of such chains
// added in a fixed order, and the order depends on the LENGTH of the reduction alone (K for Y, N for dX, M for dW and
// db): not on M, not on the row, not on the grid.  No float atomic, no workspace, outputs are overwritten.  So row m of
// Y has the same bits in a batch of 64 and in a batch of 1, and two runs are bit-equal.
//   Y:  4 waves take K / 4 each; each a chain over its k (16 at a time: k0 + 4 g + j, j outer, g inner); the four
//       partial sums are added in wave order through LDS, then the bias.
//   dX: ceil(N / 4) steps of 4 classes, split into four contiguous runs, one per wave; combined in wave order.
//   dW, db: one chain over the rows of the batch, in row order.
// A ragged edge of an OUTPUT index (rows of Y beyond M, classes beyond N) loads the last valid row again and stores
// nothing.  A ragged edge of a REDUCTION index (classes beyond N in dX, rows beyond M in dW) feeds zeros to BOTH
// operands, so a non-finite value in the clamped row cannot leak and the chain keeps its length.  No tile is skipped
// for what an operand holds: a non-finite input propagates as in the dense product.
#include "common.h"

namespace {

constexpr int THREADS = 256;
constexpr int WAVES = THREADS / HWGAT_WAVE;

__device__ __forceinline__ f32x4 mfma4(float a, float b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

// Y[M, N] = X[M, K] W[N, K]^T + bias.  One workgroup: 16 classes x (16 MT) rows; wave w reduces k in [w K/4, (w+1) K/4).
template <int MT>
__global__ __launch_bounds__(THREADS) void head_fwd_k(const float* __restrict__ X, const float* __restrict__ W,
                                                      const float* __restrict__ bias, float* __restrict__ Y,
                                                      int M, int N, int K, int ntiles) {
    __shared__ float part[WAVES - 1][MT][4][HWGAT_WAVE];
    const int wave = threadIdx.x >> 6, lane = lane_id(), g = lane >> 4, c = lane & 15;
    const int n0 = ((int)blockIdx.x % ntiles) * 16;
    const int m0 = ((int)blockIdx.x / ntiles) * (16 * MT);
    const int kq = K / WAVES, k_lo = wave * kq;
    const float* wp = W + (size_t)min(n0 + c, N - 1) * K + k_lo + 4 * g;
    const float* xp[MT];
#pragma unroll
    for (int t = 0; t < MT; ++t) xp[t] = X + (size_t)min(m0 + 16 * t + c, M - 1) * K + k_lo + 4 * g;
    f32x4 acc[MT];
#pragma unroll
    for (int t = 0; t < MT; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
    for (int k = 0; k < kq; k += 16) {
        const f32x4 wv = *reinterpret_cast<const f32x4*>(wp + k);
        f32x4 xv[MT];
#pragma unroll
        for (int t = 0; t < MT; ++t) xv[t] = *reinterpret_cast<const f32x4*>(xp[t] + k);
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int t = 0; t < MT; ++t) acc[t] = mfma4(xv[t][j], wv[j], acc[t]);
    }
    if (wave > 0) {
#pragma unroll
        for (int t = 0; t < MT; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) part[wave - 1][t][r][lane] = acc[t][r];
    }
    __syncthreads();
    if (wave > 0) return;
    const int n = n0 + c;
    const float b = (bias && n < N) ? bias[n] : 0.f;
#pragma unroll
    for (int t = 0; t < MT; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float v = acc[t][r];
#pragma unroll
            for (int w = 0; w < WAVES - 1; ++w) v += part[w][t][r][lane];
            v += b;
            const int m = m0 + 16 * t + 4 * g + r;
            if (m < M && n < N) Y[(size_t)m * N + n] = v;
        }
}

// dX[M, K] = dY[M, N] W[N, K].  One workgroup: 16 rows x 64 columns (lane c holds columns k0 + 4 c + j in accumulator j);
// wave w reduces the steps [w per, (w+1) per) of 4 classes each, per = ceil(ceil(N / 4) / 4).
__global__ __launch_bounds__(THREADS) void head_bwd_dx_k(const float* __restrict__ dY, const float* __restrict__ W,
                                                         float* __restrict__ dX, int M, int N, int K, int ktiles) {
    __shared__ float part[WAVES - 1][4][4][HWGAT_WAVE];
    const int wave = threadIdx.x >> 6, lane = lane_id(), g = lane >> 4, c = lane & 15;
    const int k0 = ((int)blockIdx.x % ktiles) * 64;
    const int m0 = ((int)blockIdx.x / ktiles) * 16;
    const int steps = (N + 3) >> 2, per = (steps + WAVES - 1) / WAVES;
    const int s_lo = wave * per, s_hi = min(steps, s_lo + per);
    const float* dyp = dY + (size_t)min(m0 + c, M - 1) * N;
    const float* wp = W + k0 + 4 * c;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    f32x4 acc[4] = {zero, zero, zero, zero};
#pragma unroll 4
    for (int s = s_lo; s < s_hi; ++s) {
        const int n = 4 * s + g, nc = min(n, N - 1);
        const bool live = n < N;
        float a = dyp[nc];
        f32x4 wv = *reinterpret_cast<const f32x4*>(wp + (size_t)nc * K);
        a = live ? a : 0.f;
        wv = live ? wv : zero;
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j] = mfma4(a, wv[j], acc[j]);
    }
    if (wave > 0) {
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) part[wave - 1][j][r][lane] = acc[j][r];
    }
    __syncthreads();
    if (wave > 0) return;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        float v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            v[j] = acc[j][r];
#pragma unroll
            for (int w = 0; w < WAVES - 1; ++w) v[j] += part[w][j][r][lane];
        }
        const int m = m0 + 4 * g + r;
        if (m < M) *reinterpret_cast<f32x4*>(dX + (size_t)m * K + k0 + 4 * c) = f32x4{v[0], v[1], v[2], v[3]};
    }
}

// dW[N, K] = dY[M, N]^T X[M, K], db[N] = column sums of dY.  One WAVE: 16 classes x 64 columns, one chain over the rows
// of the batch; the wave of a class tile's first 64 columns also sums dY itself (an MFMA against ones: the same chain, in
// row order, every product exact).
__global__ __launch_bounds__(THREADS) void head_bwd_dw_k(const float* __restrict__ dY, const float* __restrict__ X,
                                                         float* __restrict__ dW, float* __restrict__ db,
                                                         int M, int N, int K, int ktiles, int tiles) {
    const int tile = (int)blockIdx.x * WAVES + (threadIdx.x >> 6);
    if (tile >= tiles) return;                                // whole waves; the kernel has no barrier
    const int lane = lane_id(), g = lane >> 4, c = lane & 15;
    const int n0 = (tile / ktiles) * 16, k0 = (tile % ktiles) * 64;
    const bool sums = db != nullptr && k0 == 0;
    const float* dyp = dY + min(n0 + c, N - 1);
    const float* xp = X + k0 + 4 * c;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    f32x4 acc[4] = {zero, zero, zero, zero};
    f32x4 accb = zero;
    const int steps = (M + 3) >> 2;
#pragma unroll 4
    for (int s = 0; s < steps; ++s) {
        const int m = 4 * s + g, mc = min(m, M - 1);
        const bool live = m < M;
        float a = dyp[(size_t)mc * N];
        f32x4 xv = *reinterpret_cast<const f32x4*>(xp + (size_t)mc * K);
        a = live ? a : 0.f;
        xv = live ? xv : zero;
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j] = mfma4(a, xv[j], acc[j]);
        if (sums) accb = mfma4(a, 1.0f, accb);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int n = n0 + 4 * g + r;
        if (n < N) {
            *reinterpret_cast<f32x4*>(dW + (size_t)n * K + k0 + 4 * c) = f32x4{acc[0][r], acc[1][r], acc[2][r], acc[3][r]};
            if (sums && c == 0) db[n] = accb[r];
        }
    }
}

// HWGAT_EINVAL / HWGAT_ESHAPE before any HIP call; `vec` are the pointers the kernels touch with 16-byte accesses
int head_check(const void* const* req, int nreq, const void* const* vec, int nvec, int M, int N, int K) {
    for (int i = 0; i < nreq; ++i)
        if (!req[i]) return HWGAT_EINVAL;
    if (M <= 0 || N <= 0) return HWGAT_EINVAL;
    if (N > 65536 || K < 64 || K > 1024 || K % 64 != 0) return HWGAT_ESHAPE;
    if (M > 0x7fffff00) return HWGAT_ESHAPE;                  // row indices of the last tile stay inside an int
    for (int i = 0; i < nvec; ++i)
        if ((uintptr_t)vec[i] & 15) return HWGAT_EINVAL;
    return 0;
}

// a one-dimensional grid of `a * b` workgroups, or 0 when that exceeds what a launch takes
int64_t grid_of(int64_t a, int64_t b) { return a * b <= 0x7fffffffLL ? a * b : 0; }

}  // namespace

extern "C" int hwgat_head_fwd(const float* X, const float* W, const float* bias, float* Y, int M, int N, int K, void* stream) {
    const void* req[] = {X, W, Y};
    const void* vec[] = {X, W};
    if (const int rc = head_check(req, 3, vec, 2, M, N, K)) return rc;
    const int ntiles = (N + 15) / 16;
    const int mt = M > 48 ? 4 : (M + 15) / 16;                // row tiles resident in one wave: W is read once per 16 mt rows
    const int64_t grid = grid_of(ntiles, (M + 16 * mt - 1) / (16 * mt));
    if (!grid) return HWGAT_ESHAPE;
    hipStream_t st = (hipStream_t)stream;
    switch (mt) {
        case 1: head_fwd_k<1><<<(unsigned)grid, THREADS, 0, st>>>(X, W, bias, Y, M, N, K, ntiles); break;
        case 2: head_fwd_k<2><<<(unsigned)grid, THREADS, 0, st>>>(X, W, bias, Y, M, N, K, ntiles); break;
        case 3: head_fwd_k<3><<<(unsigned)grid, THREADS, 0, st>>>(X, W, bias, Y, M, N, K, ntiles); break;
        default: head_fwd_k<4><<<(unsigned)grid, THREADS, 0, st>>>(X, W, bias, Y, M, N, K, ntiles); break;
    }
    HWGAT_LAUNCH_CHECK();
}

extern "C" int hwgat_head_bwd_dx(const float* dY, const float* W, float* dX, int M, int N, int K, void* stream) {
    const void* req[] = {dY, W, dX};
    const void* vec[] = {W, dX};
    if (const int rc = head_check(req, 3, vec, 2, M, N, K)) return rc;
    const int ktiles = K / 64;
    const int64_t grid = grid_of(ktiles, (M + 15) / 16);
    if (!grid) return HWGAT_ESHAPE;
    head_bwd_dx_k<<<(unsigned)grid, THREADS, 0, (hipStream_t)stream>>>(dY, W, dX, M, N, K, ktiles);
    HWGAT_LAUNCH_CHECK();
}

extern "C" int hwgat_head_bwd_dw(const float* dY, const float* X, float* dW, float* db, int M, int N, int K, void* stream) {
    const void* req[] = {dY, X, dW};
    const void* vec[] = {X, dW};
    if (const int rc = head_check(req, 3, vec, 2, M, N, K)) return rc;
    const int ktiles = K / 64, tiles = ((N + 15) / 16) * ktiles;          // at most 4096 x 16
    head_bwd_dw_k<<<(tiles + WAVES - 1) / WAVES, THREADS, 0, (hipStream_t)stream>>>(dY, X, dW, db, M, N, K, ktiles, tiles);
    HWGAT_LAUNCH_CHECK();
}
