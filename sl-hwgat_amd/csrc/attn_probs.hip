// Attention-probability export for the five attention kinds (functional.ATTN_KINDS) on gfx950 (MI355X).
//
// The fused forwards (win / pwin / blk / band / wband) keep the softmax output P in registers and never write it.  This
// file is the diagnostic path that does: from the SAME qkv tensor and the SAME mask rows a forward reads it writes
//   probs     the eval-mode P, fp32, in the reference's attention-tensor layout (include/hwgat_hip.h), and / or
//   received  (B, F, K) fp32: the head-mean column sums of P, "how much attention this joint of this frame received",
// with no train-mode threshold and no attention dropout.  Either output alone costs no pass over the other: `received`
// never materialises P in HBM.  No atomics anywhere: every output element has exactly one writer that sums in a fixed
// order, so two runs are bit-equal and a clip's values do not depend on the batch around it.
//
// Two kernels, fp32 arithmetic on vector FMAs for both storage dtypes (bf16 is widened on load, nothing is rounded back):
//
//   pair (win, pwin, blk)   a window = n = 2 W tokens of one frame pair.  One wave serves ALL heads of G = 64 / n
//       consecutive windows, packed like pwin_attn.hip: lane l is query t = l % n of window l / n.  Per head: the keys
//       go to LDS as fp32 rows, the lane's logits / mask / "== 0 -> -10000" fill / softmax are lane-local (no cross-lane
//       reduction), the P rows go to an LDS tile that overlays the key rows, and the same lane -- now as KEY t of its
//       window -- adds its column.  A key belongs to exactly one window, so after the head loop the lane owns one
//       finished `received` value.  P leaves the tile as whole contiguous n x n blocks.
//
//   band (band, wband)      a window = W joints over all F frames; a query of frame f sees keys of frames f-1, f, f+1.
//       One 128-thread workgroup owns FS = 128 / W - 2 consecutive KEY frames of one (clip, window) and computes the
//       query rows of those frames and of the one frame on either side: FS + 2 query frames for FS key frames, i.e. the
//       halo rows' normalisers are recomputed by the neighbouring workgroup instead of being exchanged through a buffer
//       (a unit per key-frame segment, one launch, no workspace).  Thread = one query row; the rows go to an LDS tile,
//       thread (key frame, joint) then sums its column over the up to three query frames that exist.
#include "attn_common.h"

namespace {

enum { PK_WIN = HWGAT_ATTN_WIN, PK_PWIN = HWGAT_ATTN_PWIN, PK_BLK = HWGAT_ATTN_BLK, PK_BAND = HWGAT_ATTN_BAND,
       PK_WBAND = HWGAT_ATTN_WBAND };

// a token's HD-wide slice of q (or k) -> registers, times s
template <typename T, int HD>
__device__ __forceinline__ void probs_row(float (&q)[HD], const T* p, float s) {
#pragma unroll
    for (int c = 0; c < HD; c += 4) {
        float v[4];
        load_nt_s<T, 4>(p + c, v);
        q[c] = v[0] * s; q[c + 1] = v[1] * s; q[c + 2] = v[2] * s; q[c + 3] = v[3] * s;
    }
}

template <int HD>
__device__ __forceinline__ float probs_dot(const float (&q)[HD], const float* kr) {
    float a = 0.f;
#pragma unroll
    for (int c = 0; c < HD; c += 4) {
        const f32x4 k4 = *reinterpret_cast<const f32x4*>(kr + c);
        a = fmaf(q[c], k4.x, a);
        a = fmaf(q[c + 1], k4.y, a);
        a = fmaf(q[c + 2], k4.z, a);
        a = fmaf(q[c + 3], k4.w, a);
    }
    return a;
}

// =============================================================== pair kinds
struct PairGeom {
    int kind, F, K, W, n, nW, nH, f, d, shift, G, n_windows;    // n = 2 W tokens per window, G windows per wave
};

// token index of slot t (tp = t / W, joint t % W) of window `wdx` (= (b f + fi) nW + wi, the reference's B_ order):
// in a shifted block window fi holds frames (2 fi + 1) % F and (2 fi + 2) % F (torch.roll(x, -1), HWGATE.py:197-200)
__device__ __forceinline__ int64_t pair_tok(const PairGeom& g, int wdx, int t) {
    const int wi = wdx % g.nW;
    const int t2 = wdx / g.nW;
    const int fi = t2 % g.f;
    const int b = t2 / g.f;
    const int tp = t >= g.W ? 1 : 0;
    int fr = 2 * fi + tp + g.shift;
    if (fr >= g.F) fr -= g.F;
    return ((int64_t)b * g.F + fr) * g.K + wi * g.W + (t - tp * g.W);
}

// bit j = key slot j visible to query slot t, from the kind's own mask format; the last window of a shifted block takes
// the same-frame rows (mask[1])
__device__ __forceinline__ uint64_t pair_mrow(const void* mask, const PairGeom& g, int wdx, int t) {
    const int wi = wdx % g.nW;
    const int fi = (wdx / g.nW) % g.f;
    const int sel = (g.shift && fi == g.f - 1) ? 1 : 0;
    if (g.kind == PK_PWIN) return static_cast<const uint64_t*>(mask)[((int64_t)sel * g.nW + wi) * g.n + t];
    if (g.kind == PK_WIN) return static_cast<const uint32_t*>(mask)[((int64_t)sel * g.nW + wi) * 32 + t];
    const int tp = t >= g.W ? 1 : 0;                       // blk: (2, 64, 2) words, query slot tp * 32 + joint
    const uint32_t* m = static_cast<const uint32_t*>(mask) + ((sel * 64 + tp * 32 + (t - tp * g.W)) * 2);
    const uint64_t low = g.W >= 32 ? 0xffffffffull : ((1ull << g.W) - 1ull);
    return ((uint64_t)m[0] & low) | (((uint64_t)m[1] & low) << g.W);
}

template <typename T, int HD, int NMAX>
__global__ __launch_bounds__(64) void attn_probs_pair_k(const T* __restrict__ qkv, const void* __restrict__ mask,
                                                        float* __restrict__ probs, float* __restrict__ received,
                                                        PairGeom g) {
    constexpr int LDW = HD + 4;                 // key rows: 16-byte padding, packed windows' rows hit other banks
    constexpr int LDP = NMAX + 1;               // P tile: a lane writes its row, reads its column
    constexpr int KS = 64 * LDW, PS = 64 * LDP;
    constexpr int EPV = 16 / sizeof(T), CPR = HD / EPV;
    __shared__ __attribute__((aligned(16))) float tile[KS > PS ? KS : PS];    // keys, then P, of one head
    const int lane = threadIdx.x;
    const int n = g.n;
    const int wdx0 = blockIdx.x * g.G;
    const int nwin = min(g.G, g.n_windows - wdx0);
    const int rows = nwin * n;
    const bool live = lane < rows;
    const int gi = live ? lane / n : 0;
    const int t = live ? lane - gi * n : 0;
    const int wdx = wdx0 + gi;
    const int64_t tok = pair_tok(g, wdx, t);
    const uint64_t mrow = live ? pair_mrow(mask, g, wdx, t) : 0ull;
    const int64_t row3d = 3 * (int64_t)g.d;
    float acc = 0.f;
    for (int h = 0; h < g.nH; ++h) {
        for (int idx = lane; idx < rows * CPR; idx += 64) {
            const int r = idx / CPR, c = idx - r * CPR;
            const int g2 = r / n;
            const int64_t tk = pair_tok(g, wdx0 + g2, r - g2 * n);
            chunk<T>::to_lds(tile + r * LDW + c * EPV, load16_s(qkv + tk * row3d + g.d + h * HD + c * EPV), 1.0f);
        }
        float q[HD];
        if (live) probs_row<T, HD>(q, qkv + tok * row3d + h * HD, qk_scale<HD>());       // q pre-scaled, HWGATE.py:89
        __syncthreads();
        float s[NMAX];
        if (live) {
            const float* kr = tile + gi * n * LDW;
            float m = -3.0e38f;
#pragma unroll
            for (int j = 0; j < NMAX; ++j) {
                if (j < n) {
                    float v = probs_dot<HD>(q, kr + j * LDW);
                    v = ((mrow >> j) & 1ull) ? v : 0.f;               // multiplicative masks, HWGATE.py:102-108
                    if (v == 0.f) v = -10000.f;                       // HWGATE.py:110, a genuinely zero product included
                    s[j] = v;
                    m = fmaxf(m, v);
                }
            }
            float sum = 0.f;
#pragma unroll
            for (int j = 0; j < NMAX; ++j) if (j < n) { s[j] = sm_exp(s[j] - m); sum += s[j]; }
            const float inv = 1.0f / sum;
#pragma unroll
            for (int j = 0; j < NMAX; ++j) if (j < n) s[j] *= inv;
        }
        __syncthreads();                                              // every lane is done with the keys
        if (live) {
#pragma unroll
            for (int j = 0; j < NMAX; ++j) if (j < n) tile[lane * LDP + j] = s[j];
        }
        __syncthreads();
        if (live) {                                                   // the lane as key t of its window: its column
            const float* pc = tile + gi * n * LDP + t;
            for (int i = 0; i < n; ++i) acc += pc[i * LDP];
        }
        if (probs) {
            const int nn = n * n;
            for (int g2 = 0; g2 < nwin; ++g2) {
                float* dst = probs + ((int64_t)(wdx0 + g2) * g.nH + h) * nn;
                const float* src = tile + g2 * n * LDP;
                for (int idx = lane; idx < nn; idx += 64) {
                    const int i = idx / n;
                    dst[idx] = src[i * LDP + (idx - i * n)];
                }
            }
        }
        __syncthreads();
    }
    if (received && live) received[tok] = acc / (float)g.nH;
}

// =============================================================== band kinds
struct BandGeom {
    int kind, F, K, W, nW, nH, d, FS, nseg;     // FS key frames per workgroup, nseg workgroups per (clip, window)
};

template <typename T, int HD, int NW>
__global__ __launch_bounds__(128) void attn_probs_band_k(const T* __restrict__ qkv, const void* __restrict__ mask,
                                                         float* __restrict__ probs, float* __restrict__ received,
                                                         BandGeom g) {
    constexpr int LDW = HD + 4;
    constexpr int LDP = 3 * NW + 1;
    constexpr int KROWS = 128 + 2 * NW;         // (FS + 4) W <= 128 + 2 W key rows: frames f0 - 2 .. f0 + FS + 1
    constexpr int EPV = 16 / sizeof(T), CPR = HD / EPV;
    __shared__ __attribute__((aligned(16))) float Ks[KROWS * LDW];
    __shared__ float Ps[128 * LDP];             // row = query (frame f0 - 1 + r / W, joint r % W), column = t W + key joint
    const int tid = threadIdx.x;
    const int W = g.W, F = g.F;
    int u = blockIdx.x;
    const int seg = u % g.nseg; u /= g.nseg;
    const int w = u % g.nW;
    const int b = u / g.nW;
    const int f0 = seg * g.FS;
    const int fs = min(g.FS, F - f0);           // this workgroup's key frames [f0, f0 + fs)
    const int qrows = (fs + 2) * W;
    const int qf = tid / W, qi = tid - qf * W;
    const int fq = f0 - 1 + qf;
    const bool qlive = tid < qrows && fq >= 0 && fq < F;
    const bool klive = tid < fs * W;            // as a key: frame f0 + qf, joint qi
    const int fk_own = f0 + qf;
    uint32_t mw[3] = {0u, 0u, 0u};
    if (qlive) {
        if (g.kind == PK_BAND) {
            const uint64_t row = static_cast<const uint64_t*>(mask)[w * 16 + qi];
            mw[0] = (uint32_t)(row & 0xffffull); mw[1] = (uint32_t)((row >> 16) & 0xffffull); mw[2] = (uint32_t)((row >> 32) & 0xffffull);
        } else {
            const uint32_t* m = static_cast<const uint32_t*>(mask) + (w * 32 + qi) * 3;
            mw[0] = m[0]; mw[1] = m[1]; mw[2] = m[2];
        }
#pragma unroll
        for (int t = 0; t < 3; ++t) {           // key frames outside the clip do not exist
            const int fk = fq - 1 + t;
            if (fk < 0 || fk >= F) mw[t] = 0u;
        }
    }
    const int64_t row3d = 3 * (int64_t)g.d;
    const int nk = (fs + 4) * W;
    float acc = 0.f;
    for (int h = 0; h < g.nH; ++h) {
        for (int idx = tid; idx < nk * CPR; idx += 128) {
            const int r = idx / CPR, c = idx - r * CPR;
            const int kf = r / W;
            const int fk = f0 - 2 + kf;
            if (fk >= 0 && fk < F) {
                const int64_t tk = ((int64_t)b * F + fk) * g.K + w * W + (r - kf * W);
                chunk<T>::to_lds(Ks + r * LDW + c * EPV, load16_s(qkv + tk * row3d + g.d + h * HD + c * EPV), 1.0f);
            }
        }
        float q[HD];
        if (qlive) probs_row<T, HD>(q, qkv + (((int64_t)b * F + fq) * g.K + w * W + qi) * row3d + h * HD, qk_scale<HD>());
        __syncthreads();
        if (qlive) {
            float s[3 * NW];
            float m = -3.0e38f;
#pragma unroll
            for (int t = 0; t < 3; ++t) {
                const float* kr = Ks + (qf + t) * W * LDW;            // key frame fq - 1 + t = f0 - 2 + (qf + t)
#pragma unroll
                for (int j = 0; j < NW; ++j) {
                    if (j < W) {
                        const float v = probs_dot<HD>(q, kr + j * LDW);   // rows of frames outside the clip: never selected
                        s[t * NW + j] = ((mw[t] >> j) & 1u) ? v : -3.0e38f;
                        m = fmaxf(m, s[t * NW + j]);
                    }
                }
            }
            float sum = 0.f;
#pragma unroll
            for (int t = 0; t < 3; ++t)
#pragma unroll
                for (int j = 0; j < NW; ++j)
                    if (j < W) {
                        const float e = ((mw[t] >> j) & 1u) ? sm_exp(s[t * NW + j] - m) : 0.f;   // masked: exp(s - 10000 - max) = 0 in fp32
                        s[t * NW + j] = e;
                        sum += e;
                    }
            const float inv = sum > 0.f ? 1.0f / sum : 0.f;           // a row without any visible key: zeros, as the forward
            float* pr = Ps + tid * LDP;
#pragma unroll
            for (int t = 0; t < 3; ++t)
#pragma unroll
                for (int j = 0; j < NW; ++j)
                    if (j < W) pr[t * W + j] = s[t * NW + j] * inv;
        }
        __syncthreads();
        if (klive) {                                                  // key (fk_own, qi): query frames fk_own + 1 - t, t = 0, 1, 2
#pragma unroll
            for (int t = 0; t < 3; ++t) {
                const int fqq = fk_own + 1 - t;
                if (fqq >= 0 && fqq < F) {
                    const float* pc = Ps + (fqq - f0 + 1) * W * LDP + t * W + qi;
                    for (int i = 0; i < W; ++i) acc += pc[i * LDP];
                }
            }
        }
        if (probs) {                                                  // the owned query frames: one contiguous run of rows
            const int w3 = 3 * W;
            const int count = fs * W * w3;
            float* dst = probs + (((((int64_t)b * g.nW + w) * g.nH + h) * F + f0) * W) * w3;
            for (int idx = tid; idx < count; idx += 128) {
                const int r = idx / w3;
                dst[idx] = Ps[(W + r) * LDP + (idx - r * w3)];
            }
        }
        __syncthreads();
    }
    if (received && klive) received[((int64_t)b * F + fk_own) * g.K + w * W + qi] = acc / (float)g.nH;
}

// ---- launchers
bool probs_is_pair(int kind) { return kind == PK_WIN || kind == PK_PWIN || kind == PK_BLK; }

// the shapes the kind's own forward accepts
bool probs_shape_ok(int kind, int B, int F, int K, int W, int nH, int hd, bool check_hd) {
    if (kind < PK_WIN || kind > PK_WBAND) return false;
    if (B <= 0 || F <= 0 || K <= 0 || W < 1 || W > 32 || K % W || nH <= 0) return false;
    if (probs_is_pair(kind) && F % 2) return false;
    if ((kind == PK_WIN || kind == PK_BAND) && W != 16) return false;
    if (kind == PK_BLK && W != K) return false;
    if (!check_hd) return true;
    if (kind == PK_WIN) return hd == 32 || hd == 64 || hd == 128;
    if (kind == PK_PWIN || kind == PK_BLK) return hd == 32 || hd == 64;
    return hd == 16 || hd == 32;
}

template <typename T, int HD>
int pair_launch(const void* qkv, const void* mask, float* probs, float* received, const PairGeom& g, hipStream_t st) {
    const int blocks = (g.n_windows + g.G - 1) / g.G;
    const T* x = static_cast<const T*>(qkv);
    if (g.n <= 32) attn_probs_pair_k<T, HD, 32><<<blocks, 64, 0, st>>>(x, mask, probs, received, g);
    else if constexpr (HD <= 64) attn_probs_pair_k<T, HD, 64><<<blocks, 64, 0, st>>>(x, mask, probs, received, g);
    else return HWGAT_ESHAPE;
    HWGAT_LAUNCH_CHECK();
}

template <typename T, int HD>
int band_launch(const void* qkv, const void* mask, float* probs, float* received, const BandGeom& g, int B, hipStream_t st) {
    const int64_t blocks = (int64_t)B * g.nW * g.nseg;
    if (blocks > 0x7fffffff) return HWGAT_ESHAPE;
    const T* x = static_cast<const T*>(qkv);
    if (g.W <= 16) attn_probs_band_k<T, HD, 16><<<(int)blocks, 128, 0, st>>>(x, mask, probs, received, g);
    else attn_probs_band_k<T, HD, 32><<<(int)blocks, 128, 0, st>>>(x, mask, probs, received, g);
    HWGAT_LAUNCH_CHECK();
}

}  // namespace

extern "C" int64_t hwgat_attn_probs_numel(int kind, int B, int F, int K, int W, int nH) {
    if (!probs_shape_ok(kind, B, F, K, W, nH, 0, false)) return 0;
    const int64_t nW = K / W;
    if (probs_is_pair(kind)) return (int64_t)B * (F / 2) * nW * nH * (2 * W) * (2 * W);
    return (int64_t)B * nW * nH * F * W * 3 * W;
}

extern "C" int hwgat_attn_probs(int kind, const void* qkv, const void* mask, float* probs, float* received, int B, int F,
                                int K, int W, int nH, int hd, int shifted, int dtype, void* stream) {
    if (!probs_shape_ok(kind, B, F, K, W, nH, hd, true)) return HWGAT_ESHAPE;       // shapes first: no pointer is touched
    if (dtype != HWGAT_F32 && dtype != HWGAT_BF16) return HWGAT_EDTYPE;
    if (!qkv || !mask || (!probs && !received)) return HWGAT_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    if (probs_is_pair(kind)) {
        const int64_t windows = (int64_t)B * (F / 2) * (K / W);
        if (windows > 0x7fffffff) return HWGAT_ESHAPE;
        const int n = 2 * W;
        const PairGeom g{kind, F, K, W, n, K / W, nH, F / 2, nH * hd, shifted ? 1 : 0, 64 / n, (int)windows};
#define PROBS_PAIR(T)                                                                       \
        (hd == 32 ? pair_launch<T, 32>(qkv, mask, probs, received, g, st)                   \
         : hd == 64 ? pair_launch<T, 64>(qkv, mask, probs, received, g, st)                 \
         : pair_launch<T, 128>(qkv, mask, probs, received, g, st))
        return dtype == HWGAT_F32 ? PROBS_PAIR(float) : PROBS_PAIR(bf16_t);
#undef PROBS_PAIR
    }
    const int FS = 128 / W - 2;
    const BandGeom g{kind, F, K, W, K / W, nH, nH * hd, FS, (F + FS - 1) / FS};
#define PROBS_BAND(T)                                                                       \
    (hd == 16 ? band_launch<T, 16>(qkv, mask, probs, received, g, B, st)                    \
     : band_launch<T, 32>(qkv, mask, probs, received, g, B, st))
    return dtype == HWGAT_F32 ? PROBS_BAND(float) : PROBS_BAND(bf16_t);
#undef PROBS_BAND
}
