// Weight / bias gradients of the linears whose dW is an odd multiple of 64 wide or tall (N % 128 == 64 or
// K % 128 == 64): the qkv, proj, fc1 and fc2 backward of HWGATE stages of width 64, 192, ... (reference
// hwgat/models/HWGATE.py:86,115,131,134 backward), fp32 and bf16 operands.
//
//  tn64_k   dW[N,K] = A[M,N]^T . B[M,K] over one M split, db[N] = colsum(A) over the split; 64x64 dW tile per block,
//           4 waves x one 32x32 tile, 32-row stages double-buffered in LDS (fp32 rows padded to 96 floats: the two
//           k-halves of a v_mfma_f32_32x32x2_f32 operand land in disjoint bank halves).  bf16 operands are widened
//           exactly to fp32 in the loader; the prologue results (dropout mask on A, LayerNorm of B) are rounded to bf16
//           as the 128x128 bf16 kernel rounds them.  Prologues as gemm_tn_k: dropout mask on A (element index m*N+n),
//           LayerNorm of B on the fly.
//  tn64_reduce_k   adds the splits' partial images in a fixed order.
//
// No float atomics: a split stores its partial tile, and the reduction order depends on the shape only, so the result
// is bit-reproducible and the same launch serves the plain, `_ws` and `_det` entry points.
#include "common.h"
#include "fused_ops.h"
#include "gemm_tn64.h"

namespace {

constexpr int BT = 64;        // dW tile edge
constexpr int TM = 32;        // rows of M per LDS stage
constexpr int LDR = 96;       // LDS row stride (floats)

struct Tn64Args {
    const void* A; const void* B; float* dW; float* db;
    float* ws;                // NULL: one split, dW / db += the tile; else images of n_split x (N K) then n_split x N
    const float* mean; const float* rstd; const float* gamma; const float* beta;
    int64_t M; int N, K;
    int n_split; int64_t rows_per_split;
    uint32_t pro_seed; float pro_p;
    const uint32_t* seed_base;
};

__device__ __forceinline__ void ld8(const float* p, float (&v)[8]) {
    const f32x4 a = *reinterpret_cast<const f32x4*>(p), b = *reinterpret_cast<const f32x4*>(p + 4);
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
}
__device__ __forceinline__ void ld8(const bf16_t* p, float (&v)[8]) {
    const bf16x8 a = *reinterpret_cast<const bf16x8*>(p);
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = (float)a[e];
}

template <typename T, bool DROP, bool BLN>
__global__ __launch_bounds__(256, 2) void tn64_k(Tn64Args p) {
    const uint32_t seed = p.pro_seed + (DROP ? seed_base_of(p.seed_base) : 0u);
    __shared__ __attribute__((aligned(16))) float sm[2 * 2 * TM * LDR];      // [buf][A|B][TM][LDR]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lq = lane & 31, hh = lane >> 5;
    const int wn = wave >> 1, wk = wave & 1;
    const int tiles_k = p.K / BT, n_tiles = (p.N / BT) * tiles_k;
    const int tile = blockIdx.x % n_tiles, split = blockIdx.x / n_tiles;
    const int n0 = (tile / tiles_k) * BT, k0 = (tile % tiles_k) * BT;
    const int64_t r_begin = (int64_t)split * p.rows_per_split;
    const int64_t r_end = r_begin + p.rows_per_split < p.M ? r_begin + p.rows_per_split : p.M;
    const int n_it = r_end > r_begin ? (int)((r_end - r_begin + TM - 1) / TM) : 0;   // an empty split still stores zeros
    const int64_t m_last = p.M - 1;
    const int lrow = tid >> 3, lc8 = (tid & 7) * 8;            // staged row lrow of a stage, columns lc8..lc8+7
    const uint32_t th = drop_thresh(p.pro_p);
    const float sc = 1.0f / (1.0f - p.pro_p);
    const T* Ag = static_cast<const T*>(p.A);
    const T* Bg = static_cast<const T*>(p.B);

    float ra[8], rb[8], colsum[8], lg[8], lb[8];
    float bm = 0.f, bs = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) { colsum[e] = 0.f; lg[e] = 1.f; lb[e] = 0.f; }
    if constexpr (BLN) {
#pragma unroll
        for (int e = 0; e < 8; ++e) { lg[e] = p.gamma[k0 + lc8 + e]; lb[e] = p.beta[k0 + lc8 + e]; }
    }
    // rows past the end of the split are rows of the next split (or past M): the last stage of a split is partial only
    // when the split ends at M, so `row < M` is the whole test
    auto issue = [&](int it) {
        int64_t row = r_begin + (int64_t)it * TM + lrow;
        row = row < m_last ? row : m_last;
        ld8(Ag + row * p.N + n0 + lc8, ra);
        ld8(Bg + row * p.K + k0 + lc8, rb);
        if constexpr (BLN) { bm = p.mean[row]; bs = p.rstd[row]; }
    };
    auto commit = [&](int buf, int it) {
        float* As = sm + buf * (2 * TM * LDR);
        float* Bs = As + TM * LDR;
        const int64_t row = r_begin + (int64_t)it * TM + lrow;
        float a[8], b[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) { a[e] = ra[e]; b[e] = rb[e]; }
        if constexpr (DROP) {
            const uint64_t e0 = (uint64_t)row * p.N + n0 + lc8;
            const f32x4 k0v = drop_keep4(seed, e0, th, sc), k1v = drop_keep4(seed, e0 + 4, th, sc);
            a[0] *= k0v.x; a[1] *= k0v.y; a[2] *= k0v.z; a[3] *= k0v.w;
            a[4] *= k1v.x; a[5] *= k1v.y; a[6] *= k1v.z; a[7] *= k1v.w;
        }
        if constexpr (BLN) {
#pragma unroll
            for (int e = 0; e < 8; ++e) b[e] = (b[e] - bm) * bs * lg[e] + lb[e];
        }
        if (row > m_last) {
#pragma unroll
            for (int e = 0; e < 8; ++e) { a[e] = 0.f; b[e] = 0.f; }
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) colsum[e] += a[e];
        if constexpr (sizeof(T) == 2) {                         // the operands the bf16 kernels multiply
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                if constexpr (DROP) a[e] = (float)(bf16_t)a[e];
                if constexpr (BLN) b[e] = (float)(bf16_t)b[e];
            }
        }
        *reinterpret_cast<f32x4*>(As + lrow * LDR + lc8) = f32x4{a[0], a[1], a[2], a[3]};
        *reinterpret_cast<f32x4*>(As + lrow * LDR + lc8 + 4) = f32x4{a[4], a[5], a[6], a[7]};
        *reinterpret_cast<f32x4*>(Bs + lrow * LDR + lc8) = f32x4{b[0], b[1], b[2], b[3]};
        *reinterpret_cast<f32x4*>(Bs + lrow * LDR + lc8 + 4) = f32x4{b[4], b[5], b[6], b[7]};
    };

    f32x16 acc;
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = 0.f;
    if (n_it > 0) {
        issue(0);
        commit(0, 0);
    }
    __syncthreads();
    int buf = 0;
    for (int it = 0; it < n_it; ++it) {
        const bool have_next = it + 1 < n_it;
        if (have_next) issue(it + 1);
        // operand lanes: (column = lane & 31, row of the k-pair = lane >> 5), 2 rows of m per MFMA
        const float* As = sm + buf * (2 * TM * LDR) + wn * 32 + lq;
        const float* Bs = sm + buf * (2 * TM * LDR) + TM * LDR + wk * 32 + lq;
#pragma unroll
        for (int s = 0; s < TM / 2; ++s)
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(As[(2 * s + hh) * LDR], Bs[(2 * s + hh) * LDR], acc, 0, 0, 0);
        if (have_next) commit(buf ^ 1, it + 1);
        __syncthreads();
        buf ^= 1;
    }
    // D: lane (k = lq, hh), reg r -> dW[n = crow(r, hh)][k]
    float* img = p.ws ? p.ws + (int64_t)split * p.N * p.K : p.dW;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int n = n0 + wn * 32 + crow(r, hh);
        const int k = k0 + wk * 32 + lq;
        const int64_t idx = (int64_t)n * p.K + k;
        if (p.ws) img[idx] = acc[r];
        else img[idx] += acc[r];
    }
    if (p.db != nullptr && k0 == 0) {                           // one k-tile column owns the bias gradient
        float* red = sm;                                        // [TM][BT] partial column sums
        __syncthreads();
#pragma unroll
        for (int e = 0; e < 8; ++e) red[lrow * BT + lc8 + e] = colsum[e];
        __syncthreads();
        if (tid < BT) {
            float s = 0.f;
#pragma unroll
            for (int q = 0; q < TM; ++q) s += red[q * BT + tid];
            if (p.ws) p.ws[(int64_t)p.n_split * p.N * p.K + (int64_t)split * p.N + n0 + tid] = s;
            else p.db[n0 + tid] += s;
        }
    }
}

// out[i] += sum over s < n_img of img[s * stride + i], in a fixed order: 16 lanes per output each add every 16th image
// (ascending), then the 16 partial sums are added in lane order.  16 outputs per block.
__global__ __launch_bounds__(256) void tn64_reduce_k(const float* __restrict__ img, float* __restrict__ out, int n_img,
                                                     int64_t stride, int64_t count) {
    __shared__ float part[16][17];
    const int g = threadIdx.x >> 4, o = threadIdx.x & 15;
    const int64_t i = (int64_t)blockIdx.x * 16 + o;
    float s = 0.f;
    if (i < count)
        for (int sp = g; sp < n_img; sp += 16) s += img[sp * stride + i];
    part[g][o] = s;
    __syncthreads();
    if (g == 0 && i < count) {
        float t = 0.f;
#pragma unroll
        for (int q = 0; q < 16; ++q) t += part[q][o];
        out[i] += t;
    }
}

// M splits and rows per split: about two blocks per CU in one round, every split at least 16 stages deep
int tn64_splits(int64_t M, int N, int K, int64_t& rows) {
    const int64_t n_tiles = (int64_t)(N / BT) * (K / BT);
    int64_t want = (512 + n_tiles - 1) / n_tiles;
    const int64_t max_split = M / (TM * 16) > 0 ? M / (TM * 16) : 1;
    if (want > max_split) want = max_split;
    if (want < 1) want = 1;
    rows = (M + want - 1) / want;
    rows = (rows + TM - 1) / TM * TM;
    return (int)((M + rows - 1) / rows);
}

}  // namespace

int64_t hwgat_tn64_ws_bytes(int64_t M, int N, int K) {
    if (M <= 0 || !hwgat_tn64_takes(N, K)) return 0;
    int64_t rows;
    const int n_split = tn64_splits(M, N, K, rows);
    return (int64_t)n_split * ((int64_t)N * K + N) * 4;
}

int hwgat_tn64_run(int dtype, const void* A, const void* B, float* dW, float* db, int64_t M, int N, int K, uint32_t pro_seed,
                   float pro_p, const float* mean, const float* rstd, const float* gamma, const float* beta,
                   const uint32_t* seed_base, float* ws, int64_t ws_bytes, hipStream_t st) {
    if (!A || !B || !dW || M <= 0 || N <= 0 || K <= 0) return HWGAT_EINVAL;
    if (mean && (!rstd || !gamma || !beta)) return HWGAT_EINVAL;
    if (pro_p < 0.f || pro_p >= 1.f) return HWGAT_EINVAL;
    if (dtype != HWGAT_F32 && dtype != HWGAT_BF16) return HWGAT_EDTYPE;
    if (!hwgat_tn64_takes(N, K)) return HWGAT_ESHAPE;
    Tn64Args a{A, B, dW, db, nullptr, mean, rstd, gamma, beta, M, N, K, 1, M, pro_seed, pro_p, seed_base};
    if (ws) {
        if (ws_bytes < hwgat_tn64_ws_bytes(M, N, K)) return HWGAT_ESHAPE;
        a.ws = ws;
        a.n_split = tn64_splits(M, N, K, a.rows_per_split);
    } else {
        a.rows_per_split = (M + TM - 1) / TM * TM;
    }
    const int64_t n_tiles = (int64_t)(N / BT) * (K / BT);
    if (n_tiles * a.n_split > 0x7fffffff) return HWGAT_ESHAPE;
    const int grid = (int)(n_tiles * a.n_split);
    const bool drop = pro_p > 0.f;
#define TN64_GO(T)                                                                        \
    if (drop) { if (mean) tn64_k<T, true, true><<<grid, 256, 0, st>>>(a);                 \
                else tn64_k<T, true, false><<<grid, 256, 0, st>>>(a); }                   \
    else { if (mean) tn64_k<T, false, true><<<grid, 256, 0, st>>>(a);                     \
           else tn64_k<T, false, false><<<grid, 256, 0, st>>>(a); }
    if (dtype == HWGAT_F32) { TN64_GO(float) }
    else { TN64_GO(bf16_t) }
#undef TN64_GO
    if (!ws) HWGAT_LAUNCH_CHECK();
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
    const int64_t nk = (int64_t)N * K;
    tn64_reduce_k<<<(unsigned)((nk + 15) / 16), 256, 0, st>>>(ws, dW, a.n_split, nk, nk);
    if (db) tn64_reduce_k<<<(unsigned)((N + 15) / 16), 256, 0, st>>>(ws + a.n_split * nk, db, a.n_split, N, N);
    HWGAT_LAUNCH_CHECK();
}
