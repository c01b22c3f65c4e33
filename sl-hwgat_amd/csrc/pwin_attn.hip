// Part-window attention for HWGATE with a general window size W (1 <= W <= 32) on gfx950 (MI355X).
//
// Same attention as win_attn.hip (reference hwgat/models/HWGATE.py:89-114 with window_partition / torch.roll as
// index math), for the window sizes that kernel does not cover: a window is joints [wi W, (wi+1) W) of the frame
// pair (2 fi, 2 fi + 1) -- after the roll by one frame in odd blocks -- so it holds n = 2 W tokens.
//
// Work unit = one wave (a one-wave workgroup) for one head of G = 64 / n consecutive windows: lane l is query
// t = l % n of window g = l / n.  Windows of W < 32 are PACKED, not padded: a W = 8 window uses 16 lanes and the
// wave serves four of them, so no lane computes logits of another window's keys (no cross-window S entries, no
// cross-window masking).  Lanes past G n (W = 7: 56 of 64) and the keys past n of a row do not exist: they are in
// no softmax, no max, no sum, no gradient and no dropout index, and nothing of them is read or written in HBM.
//
//   load        q (pre-scaled, HWGATE.py:89), k, v (and dO) of the wave's G n tokens into LDS as fp32 rows, in
//               16-byte chunks: consecutive lanes read consecutive chunks of one row
//   S row       lane-local: s[j] = q . k_j over the n keys of its own window (broadcast LDS reads), so the softmax
//               row statistics need no cross-lane reduction at all
//   softmax     the train-mode threshold drop over the n raw logits (HWGATE.py:94-100), the adjacency / shift bit
//               row, the "== 0 -> -10000" fill, the softmax, the attention dropout (HWGATE.py:102-112)
//   O = P V     lane-local again; o staged through LDS and stored as whole rows
// backward: the same rows recomputed; dq lane-local; dS and P (dropout applied) go to LDS and lane j of a window
// sums the columns for dk_j and dv_j -- fixed order, no atomics, bit-reproducible run to run.
//
// Arithmetic is fp32 (v_fma_f32) for both storage dtypes: an n x n x hd product per window is too small and too
// ragged (n = 2 .. 64) for the MFMA tiles of win_attn.hip to pay off without padding, and HBM traffic is the
// algorithmic 4 E s (fwd) / 7 E s (bwd) either way.
#include "attn_common.h"
#include "fused_ops.h"            // the dropout hash (attention dropout)

namespace {

struct PwinGeom {
    int F, K, W, n, nW, nH, f, d, shift, G, n_windows;   // n = 2 W tokens per window, G windows per wave
};

// token index of slot t (tp = t / W, joint t % W) of window `wdx` (= (b f + fi) nW + wi, the reference's B_ order)
__device__ __forceinline__ int64_t pwin_tok(const PwinGeom& g, int wdx, int t) {
    const int wi = wdx % g.nW;
    const int t2 = wdx / g.nW;
    const int fi = t2 % g.f;
    const int b = t2 / g.f;
    const int tp = t >= g.W ? 1 : 0;
    int fr = 2 * fi + tp + g.shift;                  // torch.roll(x, -shift): shifted[t] = x[(t + shift) % F]
    if (fr >= g.F) fr -= g.F;
    return ((int64_t)b * g.F + fr) * g.K + wi * g.W + (t - tp * g.W);
}

// rows [0, rows) of the wave's tokens, columns [col, col + HD) of a row-major tensor with `stride` elements per token
// (the qkv rows, or dO) -> fp32 LDS rows of stride LDW, scaled by s
template <typename T, int HD, int LDW>
__device__ __forceinline__ void pwin_load(float* dst, const T* src, int64_t stride, int col, const PwinGeom& g,
                                          int wdx0, int rows, float s, int lane) {
    constexpr int EPV = 16 / sizeof(T);
    constexpr int CPR = HD / EPV;
    for (int idx = lane; idx < rows * CPR; idx += 64) {
        const int r = idx / CPR, c = idx - r * CPR;
        const int gi = r / g.n;
        const int64_t tok = pwin_tok(g, wdx0 + gi, r - gi * g.n);
        const u32x4 raw = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(src + tok * stride + col + c * EPV));
        chunk<T>::to_lds(dst + r * LDW + c * EPV, raw, s);
    }
}

// fp32 LDS rows -> `T` rows of the output (same token map)
template <typename T, int HD, int LDW>
__device__ __forceinline__ void pwin_store(T* dst, const float* src, int64_t stride, int col, const PwinGeom& g,
                                           int wdx0, int rows, int lane) {
    constexpr int CPR = HD / 4;
    for (int idx = lane; idx < rows * CPR; idx += 64) {
        const int r = idx / CPR, c = idx - r * CPR;
        const int gi = r / g.n;
        const int64_t tok = pwin_tok(g, wdx0 + gi, r - gi * g.n);
        const f32x4 v = *reinterpret_cast<const f32x4*>(src + r * LDW + c * 4);
        const float a[4] = {v.x, v.y, v.z, v.w};
        store_nt_s<T, 4>(dst + tok * stride + col + c * 4, a);
    }
}

// logits of the lane's query row -> probabilities (in s[]); returns bit j set where the gradient flows (the logit was
// not replaced by -10000).  q: the lane's pre-scaled query row; Kr: its window's first key row in LDS.
template <int HD, int NMAX, int LDW, bool TRAIN>
__device__ __forceinline__ uint64_t pwin_softmax(float (&s)[NMAX], const float (&q)[HD], const float* Kr, int n,
                                                 uint64_t mrow, float thr) {
#pragma unroll
    for (int j = 0; j < NMAX; ++j) {
        if (j < n) {
            const float* kr = Kr + j * LDW;
            float a = 0.f;
#pragma unroll
            for (int c = 0; c < HD; c += 4) {
                const f32x4 k4 = *reinterpret_cast<const f32x4*>(kr + c);
                a = fmaf(q[c], k4.x, a);
                a = fmaf(q[c + 1], k4.y, a);
                a = fmaf(q[c + 2], k4.z, a);
                a = fmaf(q[c + 3], k4.w, a);
            }
            s[j] = a;
        }
    }
    if constexpr (TRAIN) {                                  // HWGATE.py:94-100, a softmax over the n real keys
        float m0 = -3.0e38f;
#pragma unroll
        for (int j = 0; j < NMAX; ++j) if (j < n) m0 = fmaxf(m0, s[j]);
        float e[NMAX], sum = 0.f;
#pragma unroll
        for (int j = 0; j < NMAX; ++j) if (j < n) { e[j] = sm_exp(s[j] - m0); sum += e[j]; }
        const float cut = thr * sum;                        // e / sum > thr  <=>  e > thr * sum
#pragma unroll
        for (int j = 0; j < NMAX; ++j) if (j < n && e[j] > cut) s[j] = 0.f;
    }
    uint64_t nz = 0;
    float m = -3.0e38f;
#pragma unroll
    for (int j = 0; j < NMAX; ++j) {
        if (j < n) {
            float v = ((mrow >> j) & 1ull) ? s[j] : 0.f;    // HWGATE.py:102-108
            if (v == 0.f) v = -10000.f; else nz |= 1ull << j;   // HWGATE.py:110
            s[j] = v;
            m = fmaxf(m, v);
        }
    }
    float sum = 0.f;
#pragma unroll
    for (int j = 0; j < NMAX; ++j) if (j < n) { s[j] = sm_exp(s[j] - m); sum += s[j]; }
    const float inv = 1.0f / sum;
#pragma unroll
    for (int j = 0; j < NMAX; ++j) if (j < n) s[j] *= inv;                   // HWGATE.py:111
    return nz;
}

// attention-dropout factor of P[q][j] of (window wdx, head h): element ((wdx nH + h) n + q) n + j of the reference's
// (B f nW, nH, n, n) attention tensor, hashed like every other dropout site (fused_ops.h)
__device__ __forceinline__ float pwin_keep(const AttnDrop& ad, uint64_t row0, int j) {
    return drop_keep(ad.seed, row0 + j, drop_thresh(ad.p), 1.0f / (1.0f - ad.p));
}

__device__ __forceinline__ uint64_t pwin_mrow(const uint64_t* mb, const PwinGeom& g, int wdx, int t) {
    const int wi = wdx % g.nW;
    const int fi = (wdx / g.nW) % g.f;
    const int sel = (g.shift && fi == g.f - 1) ? 1 : 0;    // the last frame pair of a shifted block: no cross-frame keys
    return mb[((int64_t)sel * g.nW + wi) * g.n + t];
}

template <int HD> constexpr int pwin_ldw() { return HD + 4; }   // 16-byte row padding: packed windows' rows hit other banks

// =============================================================== forward
template <typename T, int HD, int NMAX, bool TRAIN, bool ADROP>
__global__ __launch_bounds__(64) void pwin_attn_fwd_k(const T* __restrict__ qkv, T* __restrict__ o,
                                                      const uint64_t* __restrict__ maskbits,
                                                      const float* __restrict__ thr_p, PwinGeom g, AttnDrop ad) {
    constexpr int LDW = pwin_ldw<HD>();
    __shared__ __attribute__((aligned(16))) float Qs[64 * LDW], Ks[64 * LDW], Vs[64 * LDW];
    if constexpr (ADROP) ad.seed += seed_base_of(ad.base);
    const int lane = threadIdx.x;
    const int head = blockIdx.x % g.nH;
    const int wdx0 = (blockIdx.x / g.nH) * g.G;
    const int nwin = min(g.G, g.n_windows - wdx0);
    const int rows = nwin * g.n;
    const int64_t row3d = 3 * (int64_t)g.d;
    const int col = head * HD;
    pwin_load<T, HD, LDW>(Qs, qkv, row3d, col, g, wdx0, rows, qk_scale<HD>(), lane);
    pwin_load<T, HD, LDW>(Ks, qkv, row3d, g.d + col, g, wdx0, rows, 1.0f, lane);
    pwin_load<T, HD, LDW>(Vs, qkv, row3d, 2 * g.d + col, g, wdx0, rows, 1.0f, lane);
    __syncthreads();
    if (lane < rows) {
        const int gi = lane / g.n, t = lane - gi * g.n;
        const int wdx = wdx0 + gi;
        float q[HD];
#pragma unroll
        for (int c = 0; c < HD; c += 4) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(Qs + lane * LDW + c);
            q[c] = v.x; q[c + 1] = v.y; q[c + 2] = v.z; q[c + 3] = v.w;
        }
        float p[NMAX];
        pwin_softmax<HD, NMAX, LDW, TRAIN>(p, q, Ks + gi * g.n * LDW, g.n, pwin_mrow(maskbits, g, wdx, t),
                                           TRAIN ? *thr_p : 0.f);
        if constexpr (ADROP) {
            const uint64_t row0 = (((uint64_t)wdx * g.nH + head) * g.n + t) * g.n;
#pragma unroll
            for (int j = 0; j < NMAX; ++j) if (j < g.n) p[j] *= pwin_keep(ad, row0, j);
        }
        float acc[HD];
#pragma unroll
        for (int c = 0; c < HD; ++c) acc[c] = 0.f;
        const float* Vr = Vs + gi * g.n * LDW;
#pragma unroll
        for (int j = 0; j < NMAX; ++j) {
            if (j < g.n) {
#pragma unroll
                for (int c = 0; c < HD; c += 4) {
                    const f32x4 v = *reinterpret_cast<const f32x4*>(Vr + j * LDW + c);
                    acc[c] = fmaf(p[j], v.x, acc[c]);
                    acc[c + 1] = fmaf(p[j], v.y, acc[c + 1]);
                    acc[c + 2] = fmaf(p[j], v.z, acc[c + 2]);
                    acc[c + 3] = fmaf(p[j], v.w, acc[c + 3]);
                }
            }
        }
#pragma unroll
        for (int c = 0; c < HD; c += 4)                       // the lane's own Q row is read by no other lane
            *reinterpret_cast<f32x4*>(Qs + lane * LDW + c) = f32x4{acc[c], acc[c + 1], acc[c + 2], acc[c + 3]};
    }
    __syncthreads();
    pwin_store<T, HD, LDW>(o, Qs, g.d, col, g, wdx0, rows, lane);
}

// =============================================================== backward
template <typename T, int HD, int NMAX, bool TRAIN, bool ADROP>
__global__ __launch_bounds__(64) void pwin_attn_bwd_k(const T* __restrict__ qkv, const T* __restrict__ dO,
                                                      T* __restrict__ dqkv, const uint64_t* __restrict__ maskbits,
                                                      const float* __restrict__ thr_p, PwinGeom g, AttnDrop ad) {
    constexpr int LDW = pwin_ldw<HD>();
    constexpr int LDS = 65;                                   // dS / P rows: lane j reads column j, rows of packed windows differ in bank
    constexpr int BUF = 64 * LDW > 64 * LDS ? 64 * LDW : 64 * LDS;
    __shared__ __attribute__((aligned(16))) float Qs[BUF], Ks[BUF], Vs[BUF], Ds[BUF];
    if constexpr (ADROP) ad.seed += seed_base_of(ad.base);
    const int lane = threadIdx.x;
    const int head = blockIdx.x % g.nH;
    const int wdx0 = (blockIdx.x / g.nH) * g.G;
    const int nwin = min(g.G, g.n_windows - wdx0);
    const int rows = nwin * g.n;
    const int64_t row3d = 3 * (int64_t)g.d;
    const int col = head * HD;
    const int n = g.n;
    pwin_load<T, HD, LDW>(Qs, qkv, row3d, col, g, wdx0, rows, qk_scale<HD>(), lane);
    pwin_load<T, HD, LDW>(Ks, qkv, row3d, g.d + col, g, wdx0, rows, 1.0f, lane);
    pwin_load<T, HD, LDW>(Vs, qkv, row3d, 2 * g.d + col, g, wdx0, rows, 1.0f, lane);
    pwin_load<T, HD, LDW>(Ds, dO, g.d, col, g, wdx0, rows, 1.0f, lane);
    __syncthreads();
    const bool live = lane < rows;
    const int gi = lane / n, t = lane - gi * n;
    float ds[NMAX], pd[NMAX], dq[HD];
    if (live) {
        const int wdx = wdx0 + gi;
        float p[NMAX];
        uint64_t nz;
        {
            float q[HD];
#pragma unroll
            for (int c = 0; c < HD; c += 4) {
                const f32x4 v = *reinterpret_cast<const f32x4*>(Qs + lane * LDW + c);
                q[c] = v.x; q[c + 1] = v.y; q[c + 2] = v.z; q[c + 3] = v.w;
            }
            nz = pwin_softmax<HD, NMAX, LDW, TRAIN>(p, q, Ks + gi * n * LDW, n, pwin_mrow(maskbits, g, wdx, t),
                                                    TRAIN ? *thr_p : 0.f);
        }
        // dP[j] = (dO . v_j) x dropout factor;  dz = P (dP - sum_j P dP), zero where the logit was filled with -10000
        float dor[HD];
#pragma unroll
        for (int c = 0; c < HD; c += 4) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(Ds + lane * LDW + c);
            dor[c] = v.x; dor[c + 1] = v.y; dor[c + 2] = v.z; dor[c + 3] = v.w;
        }
        const uint64_t row0 = (((uint64_t)wdx * g.nH + head) * n + t) * n;
        const float* Vr = Vs + gi * n * LDW;
        float rowdot = 0.f;
#pragma unroll
        for (int j = 0; j < NMAX; ++j) {
            if (j < n) {
                float a = 0.f;
#pragma unroll
                for (int c = 0; c < HD; c += 4) {
                    const f32x4 v = *reinterpret_cast<const f32x4*>(Vr + j * LDW + c);
                    a = fmaf(dor[c], v.x, a);
                    a = fmaf(dor[c + 1], v.y, a);
                    a = fmaf(dor[c + 2], v.z, a);
                    a = fmaf(dor[c + 3], v.w, a);
                }
                const float kp = ADROP ? pwin_keep(ad, row0, j) : 1.f;
                pd[j] = p[j] * kp;
                ds[j] = a * kp;
                rowdot = fmaf(p[j], ds[j], rowdot);
            }
        }
#pragma unroll
        for (int j = 0; j < NMAX; ++j)
            if (j < n) ds[j] = ((nz >> j) & 1ull) ? p[j] * (ds[j] - rowdot) : 0.f;
        // dq = hd^-0.5 sum_j dz_j k_j
#pragma unroll
        for (int c = 0; c < HD; ++c) dq[c] = 0.f;
        const float* Kr = Ks + gi * n * LDW;
#pragma unroll
        for (int j = 0; j < NMAX; ++j) {
            if (j < n) {
#pragma unroll
                for (int c = 0; c < HD; c += 4) {
                    const f32x4 k4 = *reinterpret_cast<const f32x4*>(Kr + j * LDW + c);
                    dq[c] = fmaf(ds[j], k4.x, dq[c]);
                    dq[c + 1] = fmaf(ds[j], k4.y, dq[c + 1]);
                    dq[c + 2] = fmaf(ds[j], k4.z, dq[c + 2]);
                    dq[c + 3] = fmaf(ds[j], k4.w, dq[c + 3]);
                }
            }
        }
#pragma unroll
        for (int c = 0; c < HD; ++c) dq[c] *= qk_scale<HD>();
    }
    __syncthreads();                                          // every lane is done with K and V
    float* Ss = Ks;                                           // dz rows, [64][LDS]
    float* Ps = Vs;                                           // dropped-out P rows, [64][LDS]
    if (live) {
#pragma unroll
        for (int j = 0; j < NMAX; ++j)
            if (j < n) { Ss[lane * LDS + j] = ds[j]; Ps[lane * LDS + j] = pd[j]; }
    }
    __syncthreads();
    float dk[HD], dv[HD];
    if (live) {                                               // lane = key t of window gi: column sums in query order
#pragma unroll
        for (int c = 0; c < HD; ++c) { dk[c] = 0.f; dv[c] = 0.f; }
        const int r0 = gi * n;
        for (int i = 0; i < n; ++i) {
            const float a = Ss[(r0 + i) * LDS + t], b = Ps[(r0 + i) * LDS + t];
            const float* qr = Qs + (r0 + i) * LDW;
            const float* dr = Ds + (r0 + i) * LDW;
#pragma unroll
            for (int c = 0; c < HD; c += 4) {
                const f32x4 q4 = *reinterpret_cast<const f32x4*>(qr + c);      // pre-scaled q: dk = sum_i dz_ij hd^-0.5 q_i
                const f32x4 d4 = *reinterpret_cast<const f32x4*>(dr + c);
                dk[c] = fmaf(a, q4.x, dk[c]); dk[c + 1] = fmaf(a, q4.y, dk[c + 1]);
                dk[c + 2] = fmaf(a, q4.z, dk[c + 2]); dk[c + 3] = fmaf(a, q4.w, dk[c + 3]);
                dv[c] = fmaf(b, d4.x, dv[c]); dv[c + 1] = fmaf(b, d4.y, dv[c + 1]);
                dv[c + 2] = fmaf(b, d4.z, dv[c + 2]); dv[c + 3] = fmaf(b, d4.w, dv[c + 3]);
            }
        }
    }
    __syncthreads();                                          // every lane is done with dz, P, q and dO
    if (live) {
#pragma unroll
        for (int c = 0; c < HD; c += 4) {
            *reinterpret_cast<f32x4*>(Ks + lane * LDW + c) = f32x4{dq[c], dq[c + 1], dq[c + 2], dq[c + 3]};
            *reinterpret_cast<f32x4*>(Vs + lane * LDW + c) = f32x4{dk[c], dk[c + 1], dk[c + 2], dk[c + 3]};
            *reinterpret_cast<f32x4*>(Qs + lane * LDW + c) = f32x4{dv[c], dv[c + 1], dv[c + 2], dv[c + 3]};
        }
    }
    __syncthreads();
    pwin_store<T, HD, LDW>(dqkv, Ks, row3d, col, g, wdx0, rows, lane);
    pwin_store<T, HD, LDW>(dqkv, Vs, row3d, g.d + col, g, wdx0, rows, lane);
    pwin_store<T, HD, LDW>(dqkv, Qs, row3d, 2 * g.d + col, g, wdx0, rows, lane);
}

// ---- launchers
bool pwin_geom(PwinGeom& g, int B, int F, int K, int W, int nH, int hd, int shifted) {
    if (B <= 0 || F <= 0 || F % 2 || K <= 0 || W < 1 || W > 32 || K % W || nH <= 0 || (hd != 32 && hd != 64))
        return false;
    const int64_t windows = (int64_t)B * (F / 2) * (K / W);
    const int n = 2 * W, G = 64 / n;
    if ((windows + G - 1) / G * nH > 0x7fffffff) return false;
    g = PwinGeom{F, K, W, n, K / W, nH, F / 2, nH * hd, shifted ? 1 : 0, G, (int)windows};
    return true;
}

template <typename T, int HD, int NMAX, bool BWD>
int pwin_launch(const void* qkv, const void* dO, void* out, const uint64_t* mb, const float* thr, const PwinGeom& g,
                AttnDrop ad, hipStream_t st) {
    const int blocks = (g.n_windows + g.G - 1) / g.G * g.nH;
    const T* x = static_cast<const T*>(qkv);
    T* y = static_cast<T*>(out);
#define PWIN_GO(TR, DR)                                                                                  \
    do {                                                                                                 \
        if constexpr (BWD)                                                                               \
            pwin_attn_bwd_k<T, HD, NMAX, TR, DR><<<blocks, 64, 0, st>>>(x, static_cast<const T*>(dO), y, mb, thr, g, ad); \
        else                                                                                             \
            pwin_attn_fwd_k<T, HD, NMAX, TR, DR><<<blocks, 64, 0, st>>>(x, y, mb, thr, g, ad);          \
    } while (0)
    if (thr && ad.p > 0.f) PWIN_GO(true, true);
    else if (thr) PWIN_GO(true, false);
    else PWIN_GO(false, false);
#undef PWIN_GO
    HWGAT_LAUNCH_CHECK();
}

template <bool BWD>
int pwin_entry(const void* qkv, const void* dO, void* out, const uint64_t* mb, const float* thr, int B, int F, int K,
               int W, int nH, int hd, int shifted, int dtype, uint32_t drop_seed, float drop_p, const uint32_t* seed_base,
               void* stream) {
    if (!qkv || !out || !mb || (BWD && !dO)) return HWGAT_EINVAL;
    if (!(drop_p >= 0.f && drop_p < 1.f) || (drop_p > 0.f && !thr)) return HWGAT_EINVAL;   // dropout: train mode only
    PwinGeom g;
    if (!pwin_geom(g, B, F, K, W, nH, hd, shifted)) return HWGAT_ESHAPE;
    if (dtype != HWGAT_F32 && dtype != HWGAT_BF16) return HWGAT_EDTYPE;
    const AttnDrop ad = make_drop(drop_seed, drop_p, seed_base);
    hipStream_t st = (hipStream_t)stream;
    const int n = 2 * W;
#define PWIN_HD(T, HD)                                                                                             \
    (n <= 8 ? pwin_launch<T, HD, 8, BWD>(qkv, dO, out, mb, thr, g, ad, st)                                         \
     : n <= 16 ? pwin_launch<T, HD, 16, BWD>(qkv, dO, out, mb, thr, g, ad, st)                                     \
     : n <= 32 ? pwin_launch<T, HD, 32, BWD>(qkv, dO, out, mb, thr, g, ad, st)                                     \
     : pwin_launch<T, HD, 64, BWD>(qkv, dO, out, mb, thr, g, ad, st))
    if (dtype == HWGAT_F32) return hd == 32 ? PWIN_HD(float, 32) : PWIN_HD(float, 64);
    return hd == 32 ? PWIN_HD(bf16_t, 32) : PWIN_HD(bf16_t, 64);
#undef PWIN_HD
}

}  // namespace

extern "C" int hwgat_pwin_attn_fwd_drop(const void* qkv, void* o, const uint64_t* maskbits, const float* thr, int B,
                                        int F, int K, int W, int nH, int hd, int shifted, int dtype, uint32_t drop_seed,
                                        float drop_p, const uint32_t* seed_base, void* stream) {
    return pwin_entry<false>(qkv, nullptr, o, maskbits, thr, B, F, K, W, nH, hd, shifted, dtype, drop_seed, drop_p,
                             seed_base, stream);
}

extern "C" int hwgat_pwin_attn_fwd(const void* qkv, void* o, const uint64_t* maskbits, const float* thr, int B, int F,
                                   int K, int W, int nH, int hd, int shifted, int dtype, void* stream) {
    return hwgat_pwin_attn_fwd_drop(qkv, o, maskbits, thr, B, F, K, W, nH, hd, shifted, dtype, 0u, 0.f, nullptr, stream);
}

extern "C" int hwgat_pwin_attn_bwd_drop(const void* qkv, const void* dO, void* dqkv, const uint64_t* maskbits,
                                        const float* thr, int B, int F, int K, int W, int nH, int hd, int shifted,
                                        int dtype, uint32_t drop_seed, float drop_p, const uint32_t* seed_base,
                                        void* stream) {
    return pwin_entry<true>(qkv, dO, dqkv, maskbits, thr, B, F, K, W, nH, hd, shifted, dtype, drop_seed, drop_p,
                            seed_base, stream);
}

extern "C" int hwgat_pwin_attn_bwd(const void* qkv, const void* dO, void* dqkv, const uint64_t* maskbits,
                                   const float* thr, int B, int F, int K, int W, int nH, int hd, int shifted, int dtype,
                                   void* stream) {
    return hwgat_pwin_attn_bwd_drop(qkv, dO, dqkv, maskbits, thr, B, F, K, W, nH, hd, shifted, dtype, 0u, 0.f, nullptr,
                                    stream);
}
