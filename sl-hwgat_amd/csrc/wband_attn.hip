// Wide band graph-attention on gfx950 (MI355X): frames of up to 32 joints.
//
// Two users: GATE (reference hwgat/models/GATE.py:40-70, one window = all K <= 32 joints of a frame) and WGATE with a
// window size other than 16 (WGATE.py:87-108).  Both references form dense (T W)^2 scores per (clip, window, head) and add
// a 0 / -10000 mask built from a block-tridiagonal adjacency (model_params.py:60-73, :209-228): a query of frame f sees
// keys of frames f-1, f, f+1 of its own window only, everything else is exp(s - 10000 - max) == 0 exactly in fp32.  The
// dense matrix never exists here:
//
//   unit  = (clip, window, frame segment, head): one wavefront walks the query frames of its segment in order; the four
//           waves of a workgroup are neighbouring heads of the same frames and stay within one frame of each other.
//   frame = 32 slots = two 16-slot halves; slots >= W are padding: their loads are clamped to the last real slot of the
//           frame (nothing outside the tensor is read), their mask rows are 0 (no probability as a key, P = dS = 0 as a
//           query) and nothing is stored for them.
//   tile  = 16 query slots x 16 key slots: one accumulator of four v_mfma_f32_16x16x4_f32 (fp32 storage) or one
//           v_mfma_f32_16x16x16_bf16 (bf16 storage) per 16 channels -- the two forms take their operands in the same lane
//           layout (lane = row, 4 consecutive contraction elements), so one kernel body serves both (struct Op).
//           12 tiles per query frame (2 query halves x 3 key frames x 2 key halves).
//   softmax over the <= 96 candidate keys in fp32 registers (24 per lane + 2 cross-lane steps); the diagonal need NOT be
//           visible (GATE has no self loops), a row without any visible key (a pad query) gets P = 0.
//   K / V tiles live in a 3-frame sliding register window: every q, k, v element is read once per segment and every o
//           element written once: 4 E s forward, 7 E s backward + the halo frames of a segment.
//   backward: P and dS are transposed through a wave-private LDS scratch (as band_attn.hip, XPOSE form); dK / dV of a key
//           frame collect query frames f-1, f, f+1 in a sliding accumulator window.  A segment owns the key frames and the
//           query frames [f0, f1) and recomputes the query frames f0-1 and f1 for their share of its dK / dV: every
//           accumulator starts at zero and receives its (up to) three contributions in the same order wherever the
//           segments are cut, so the result does not depend on the segmentation bit for bit.
//   dropout mask: the library hash over the element index of the reference's dense (B nW, nH, T W, T W) attention tensor.
#include "band_common.h"

namespace {
using namespace band;

typedef float f32x4v __attribute__((ext_vector_type(4)));
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x2v __attribute__((ext_vector_type(2)));

struct WGeom {
    int F, K, W, nW, nH, d, seg, n_seg;       // seg = owned frames per unit, n_seg = segments per clip
};
struct WUnit {
    int64_t tok0;          // token index of (clip, frame 0, first joint of the window)
    int head, w, f0, f1;   // owned frames [f0, f1)
    int bw;                // clip * nW + window
};
__device__ __forceinline__ WUnit decode_wband(const WGeom& g, int u) {
    WUnit r;
    r.head = u % g.nH;                        // heads fastest: the waves of a workgroup share 128-byte lines
    int t = u / g.nH;
    const int sgi = t % g.n_seg;
    t /= g.n_seg;
    r.bw = t;
    r.w = t % g.nW;
    r.tok0 = (int64_t)(t / g.nW) * g.F * g.K + r.w * g.W;
    r.f0 = sgi * g.seg;
    r.f1 = min(g.F, r.f0 + g.seg);
    return r;
}

// MFMA operand of 4 contraction elements per lane, and D(16x16) += A B with lane l supplying A[i = l&15][k = 4 (l>>4) + e]
// and B[k = 4 (l>>4) + e][j = l&15] (bf16) -- the fp32 form runs e = 0..3 as four k = 4 steps with k = l>>4, which
// contracts the same 16 elements; register r of lane l is D[i = 4 (l>>4) + r][j = l&15] in both.
template <typename T> struct Op;
template <> struct Op<float> {
    typedef f32x4v V;
    static constexpr bool PRE = true;         // q is scaled before the product
    __device__ static __forceinline__ V pack(const f32x4v& v) { return v; }
    __device__ static __forceinline__ V zero() { return V{0.f, 0.f, 0.f, 0.f}; }
    __device__ static __forceinline__ f32x4v mma(const V& a, const V& b, f32x4v c) {
        c = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, b.x, c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, b.y, c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, b.z, c, 0, 0, 0);
        return __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, b.w, c, 0, 0, 0);
    }
    __device__ static __forceinline__ V row4(const float* p, float mul) { return *reinterpret_cast<const f32x4v*>(p) * mul; }
};
template <> struct Op<bf16_t> {
    typedef u32x2v V;
    static constexpr bool PRE = false;        // scores are scaled in fp32 after the product: q is not rounded twice
    __device__ static __forceinline__ uint32_t pk2(float a, float b) {
        return __builtin_bit_cast(uint32_t, __builtin_convertvector(f32x2{a, b}, bf16x2));
    }
    __device__ static __forceinline__ V pack(const f32x4v& v) { return V{pk2(v.x, v.y), pk2(v.z, v.w)}; }
    __device__ static __forceinline__ V zero() { return V{0u, 0u}; }
    __device__ static __forceinline__ f32x4v mma(const V& a, const V& b, f32x4v c) {
        return __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(__builtin_bit_cast(s16x4, a), __builtin_bit_cast(s16x4, b), c, 0, 0, 0);
    }
    __device__ static __forceinline__ V row4(const bf16_t* p, float) { return *reinterpret_cast<const u32x2v*>(p); }
};

// both halves of a frame as row operands: c[h][ch] = X[slot 16 h + (l&15)][16 ch + 4 (l>>4) + 0..3]
template <typename T, int NC> struct Rows { typename Op<T>::V c[2][NC]; };
// ... as column operands: c[h][ct] = X[slot 16 h + 4 (l>>4) + 0..3][NC (l&15) + ct]
template <typename T, int NC> struct Cols { typename Op<T>::V c[2][NC]; };

struct LaneOff {
    uint32_t row[2];       // element offset of the lane's row-operand slot (clamped to W-1) + 4 (l>>4)
    uint32_t col[2][4];    // ... of its four column-operand slots (clamped) + NC (l&15)
};
template <int NC> __device__ __forceinline__ LaneOff lane_off(int W, uint32_t stride, int lr, int gq) {
    LaneOff o;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        o.row[h] = (uint32_t)min(16 * h + lr, W - 1) * stride + 4 * gq;
#pragma unroll
        for (int r = 0; r < 4; ++r) o.col[h][r] = (uint32_t)min(16 * h + 4 * gq + r, W - 1) * stride + NC * lr;
    }
    return o;
}

template <typename T, int NC>
__device__ __forceinline__ Rows<T, NC> load_rows(const T* base, const LaneOff& lo, float mul) {
    Rows<T, NC> t;
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int ch = 0; ch < NC; ++ch) t.c[h][ch] = Op<T>::row4(base + lo.row[h] + 16 * ch, mul);
    return t;
}
template <typename T, int NC>
__device__ __forceinline__ Cols<T, NC> load_cols(const T* base, const LaneOff& lo, float mul) {
    Cols<T, NC> t;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        if constexpr (sizeof(T) == 4) {
            float x[4][NC];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                if constexpr (NC == 1) x[r][0] = base[lo.col[h][r]];
                else { const f32x2 v = *reinterpret_cast<const f32x2*>(base + lo.col[h][r]); x[r][0] = v.x; x[r][1] = v.y; }
            }
#pragma unroll
            for (int ct = 0; ct < NC; ++ct) t.c[h][ct] = f32x4v{x[0][ct], x[1][ct], x[2][ct], x[3][ct]} * mul;
        } else {
            uint32_t w[4];                                       // NC bf16 of each of the four rows
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                if constexpr (NC == 1) w[r] = *reinterpret_cast<const uint16_t*>(base + lo.col[h][r]);
                else w[r] = *reinterpret_cast<const uint32_t*>(base + lo.col[h][r]);
            }
            t.c[h][0] = u32x2v{(w[0] & 0xffffu) | (w[1] << 16), (w[2] & 0xffffu) | (w[3] << 16)};
            if constexpr (NC == 2) t.c[h][1] = u32x2v{(w[0] >> 16) | (w[1] & 0xffff0000u), (w[2] >> 16) | (w[3] & 0xffff0000u)};
        }
    }
    return t;
}
// rows 16 h + 4g + r < W of a product in the column layout: acc[ct][r] = channel NC (l&15) + ct of that row
template <typename T, int NC>
__device__ __forceinline__ void store_cols(T* base, const LaneOff& lo, int h, int W, int gq, const f32x4v (&acc)[NC], float mul) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        if (16 * h + 4 * gq + r < W) {
            T* p = base + lo.col[h][r];
            if constexpr (NC == 1) *p = (T)(acc[0][r] * mul);
            else if constexpr (sizeof(T) == 4) *reinterpret_cast<f32x2*>(p) = f32x2{acc[0][r] * mul, acc[1][r] * mul};
            else *reinterpret_cast<bf16x2*>(p) = bf16x2{(bf16_t)(acc[0][r] * mul), (bf16_t)(acc[1][r] * mul)};
        }
    }
}

// D[i][j] = sum_c X[i][c] Y[j][c]: lane (j = l&15, g), register r -> D[4g + r][j]
template <typename T, int NC>
__device__ __forceinline__ f32x4v dot_rows(const typename Op<T>::V (&x)[NC], const typename Op<T>::V (&y)[NC]) {
    f32x4v acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ch = 0; ch < NC; ++ch) acc = Op<T>::mma(x[ch], y[ch], acc);
    return acc;
}
// acc[ct] += A Y with a[r] = A[i = l&15][k = 4g + r] and Y a column operand
template <typename T, int NC>
__device__ __forceinline__ void mul_cols(const f32x4v& a, const typename Op<T>::V (&y)[NC], f32x4v (&acc)[NC]) {
    const typename Op<T>::V av = Op<T>::pack(a);
#pragma unroll
    for (int ct = 0; ct < NC; ++ct) acc[ct] = Op<T>::mma(av, y[ct], acc[ct]);
}

__device__ __forceinline__ float xg_max(float v) {              // over the 4 lanes l, l^16, l^32, l^48
    v = fmaxf(v, __shfl_xor(v, 16, 64));
    return fmaxf(v, __shfl_xor(v, 32, 64));
}
__device__ __forceinline__ float xg_sum(float v) {
    v += __shfl_xor(v, 16, 64);
    return v + __shfl_xor(v, 32, 64);
}

// the lane's 4 visibility bits of every tile: nib[t][kh] bit r = key slot 16 kh + 4g + r of frame f-1+t
__device__ __forceinline__ void vis_nibbles(const uint32_t (&mw)[3], int gq, bool has_prev, bool has_next, uint32_t (&nib)[3][2]) {
#pragma unroll
    for (int t = 0; t < 3; ++t) {
        const bool ok = t == 0 ? has_prev : t == 2 ? has_next : true;
#pragma unroll
        for (int kh = 0; kh < 2; ++kh) nib[t][kh] = ok ? (mw[t] >> (16 * kh + 4 * gq)) & 0xFu : 0u;
    }
}

// probabilities of one query slot from its six key tiles; masked entries are exactly 0 (the additive -10000 of
// GATE.py:59-61 / WGATE.py:97-100 underflows to 0 in fp32); a query without a visible key (pad slot) gets zeros
__device__ __forceinline__ void wband_softmax(const f32x4v (&s)[3][2], const uint32_t (&nib)[3][2], f32x4v (&p)[3][2]) {
    float m = -3.0e38f;
#pragma unroll
    for (int t = 0; t < 3; ++t)
#pragma unroll
        for (int kh = 0; kh < 2; ++kh)
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if ((nib[t][kh] >> r) & 1u) m = fmaxf(m, s[t][kh][r]);
    m = xg_max(m);
    float sum = 0.f;
#pragma unroll
    for (int t = 0; t < 3; ++t)
#pragma unroll
        for (int kh = 0; kh < 2; ++kh)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float e = ((nib[t][kh] >> r) & 1u) ? __expf(s[t][kh][r] - m) : 0.f;
                p[t][kh][r] = e;
                sum += e;
            }
    sum = xg_sum(sum);
    const float inv = sum > 0.f ? 1.0f / sum : 0.f;
#pragma unroll
    for (int t = 0; t < 3; ++t)
#pragma unroll
        for (int kh = 0; kh < 2; ++kh) p[t][kh] *= inv;
}

// attention dropout factors of P[query row][key = (frame kf, slots 16 kh + 4g + r)]; `rowbase` = element index of the
// query's row start in the reference's dense (B nW, nH, T W, T W) tensor
__device__ __forceinline__ f32x4v wband_keep(uint32_t seed, uint64_t rowbase, int kf, int W, int kh, int gq, uint32_t thresh, float scale) {
    const uint64_t i0 = rowbase + (uint64_t)kf * W + 16 * kh + 4 * gq;
    return f32x4v{drop_keep(seed, i0, thresh, scale), drop_keep(seed, i0 + 1, thresh, scale),
                  drop_keep(seed, i0 + 2, thresh, scale), drop_keep(seed, i0 + 3, thresh, scale)};
}

// =============================================================== forward
template <typename T, int HD, int MINW, bool ADROP>
__global__ __launch_bounds__(256, MINW) void wband_attn_fwd_k(const T* __restrict__ qkv, T* __restrict__ o,
                                                              const uint32_t* __restrict__ maskrows, WGeom g, int n_units,
                                                              AttnDrop ad) {
    if constexpr (ADROP) ad.seed += seed_base_of(ad.base);
    constexpr int NC = HD / 16;
    typedef Op<T> O;
    constexpr float qmul = O::PRE ? band_scale<HD>() : 1.0f, smul = O::PRE ? 1.0f : band_scale<HD>();
    const int lane = threadIdx.x & 63, lr = lane & 15, gq = lane >> 4;
    const int u_raw = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const bool live = u_raw < n_units;                           // tail waves shadow the last unit without storing
    const WUnit un = decode_wband(g, live ? u_raw : n_units - 1);
    const int64_t rs = 3 * (int64_t)g.d, fs = (int64_t)g.K * rs, os = (int64_t)g.K * g.d;
    const T* qb = qkv + un.tok0 * rs + un.head * HD;
    T* ob = o + un.tok0 * (int64_t)g.d + un.head * HD;
    const LaneOff lq = lane_off<NC>(g.W, (uint32_t)rs, lr, gq), lo = lane_off<NC>(g.W, (uint32_t)g.d, lr, gq);
    uint32_t mw[2][3];                                           // mask words of query slots lr, 16 + lr
#pragma unroll
    for (int qh = 0; qh < 2; ++qh)
#pragma unroll
        for (int t = 0; t < 3; ++t) mw[qh][t] = maskrows[(un.w * 32 + 16 * qh + lr) * 3 + t];
    const uint32_t thresh = drop_thresh(ad.p);
    const float dscale = 1.0f / (1.0f - ad.p);
    const uint64_t TW = (uint64_t)g.F * g.W;

    // sliding window: K (row operands) and V (column operands) of frames f-1, f, f+1; loads are unconditional and
    // clamped into the clip -- tiles of frames outside it are masked out
    Rows<T, NC> kw[3];
    Cols<T, NC> vw[3];
    {
        const int fp = max(un.f0 - 1, 0);
        kw[0] = load_rows<T, NC>(qb + fp * fs + g.d, lq, 1.0f);
        vw[0] = load_cols<T, NC>(qb + fp * fs + 2 * g.d, lq, 1.0f);
        kw[1] = load_rows<T, NC>(qb + un.f0 * fs + g.d, lq, 1.0f);
        vw[1] = load_cols<T, NC>(qb + un.f0 * fs + 2 * g.d, lq, 1.0f);
    }
    Rows<T, NC> nq, nk;                                          // one frame ahead: Q of frame f, K / V of frame f + 1
    Cols<T, NC> nv;
    auto fill = [&](int f) {
        const int fq = min(f, g.F - 1), fk = min(f + 1, g.F - 1);
        nq = load_rows<T, NC>(qb + fq * fs, lq, qmul);
        nk = load_rows<T, NC>(qb + fk * fs + g.d, lq, 1.0f);
        nv = load_cols<T, NC>(qb + fk * fs + 2 * g.d, lq, 1.0f);
    };
    fill(un.f0);

    for (int it = 0; it < g.seg; ++it) {
        const int f = un.f0 + it;
        __syncthreads();                                         // neighbouring heads stay within a frame of each other
        const Rows<T, NC> q = nq;
        kw[2] = nk;
        vw[2] = nv;
        fill(f + 1);
        if (f < un.f1 && live) {
#pragma unroll
            for (int qh = 0; qh < 2; ++qh) {
                f32x4v s[3][2], p[3][2];
                uint32_t nib[3][2];
                vis_nibbles(mw[qh], gq, f > 0, f + 1 < g.F, nib);
#pragma unroll
                for (int t = 0; t < 3; ++t)
#pragma unroll
                    for (int kh = 0; kh < 2; ++kh) s[t][kh] = dot_rows<T, NC>(kw[t].c[kh], q.c[qh]) * smul;   // S[q = 16 qh + lr][key = 16 kh + 4g + r]
                wband_softmax(s, nib, p);
                if constexpr (ADROP) {                           // GATE.py:65 / WGATE.py:103
                    const uint64_t rowbase = (((uint64_t)un.bw * g.nH + un.head) * TW + (uint64_t)f * g.W + 16 * qh + lr) * TW;
#pragma unroll
                    for (int t = 0; t < 3; ++t)
#pragma unroll
                        for (int kh = 0; kh < 2; ++kh)
                            p[t][kh] *= wband_keep(ad.seed, rowbase, min(max(f - 1 + t, 0), g.F - 1), g.W, kh, gq, thresh, dscale);
                }
                f32x4v oacc[NC];
#pragma unroll
                for (int ct = 0; ct < NC; ++ct) oacc[ct] = f32x4v{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int t = 0; t < 3; ++t)
#pragma unroll
                    for (int kh = 0; kh < 2; ++kh) mul_cols<T, NC>(p[t][kh], vw[t].c[kh], oacc);
                store_cols<T, NC>(ob + f * os, lo, qh, g.W, gq, oacc, 1.0f);      // O[q = 16 qh + 4g + r][NC lr + ct]
            }
        }
        kw[0] = kw[1]; kw[1] = kw[2];
        vw[0] = vw[1]; vw[1] = vw[2];
    }
}

// =============================================================== backward
// PREF: the next query frame's tiles are fetched one frame ahead.  fp32 at head_dim 32 has no registers left for that
// (the compiler's report showed 80-103 spilled registers with it) and fetches each frame when it needs it.
template <typename T, int HD, int MINW, bool ADROP, bool PREF = !(sizeof(T) == 4 && HD == 32)>
__global__ __launch_bounds__(256, MINW) void wband_attn_bwd_k(const T* __restrict__ qkv, const T* __restrict__ dO,
                                                              T* __restrict__ dqkv, const uint32_t* __restrict__ maskrows,
                                                              WGeom g, int n_units, AttnDrop ad) {
    if constexpr (ADROP) ad.seed += seed_base_of(ad.base);
    constexpr int NC = HD / 16;
    typedef Op<T> O;
    constexpr float qmul = O::PRE ? band_scale<HD>() : 1.0f, smul = O::PRE ? 1.0f : band_scale<HD>();
    constexpr int XLD = 20;                                      // scratch row stride (floats): 16-byte aligned rows
    __shared__ __attribute__((aligned(16))) float xsm[4 * 6 * 16 * XLD];
    const int lane = threadIdx.x & 63, lr = lane & 15, gq = lane >> 4;
    const int wib = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    float* xs = xsm + wib * (6 * 16 * XLD);                      // six 16 x 16 tiles [t][kh] of P, then of dS
    const int u_raw = blockIdx.x * 4 + wib;
    const bool live = u_raw < n_units;
    const WUnit un = decode_wband(g, live ? u_raw : n_units - 1);
    const int64_t rs = 3 * (int64_t)g.d, fs = (int64_t)g.K * rs, gs = (int64_t)g.K * g.d;
    const T* qb = qkv + un.tok0 * rs + un.head * HD;
    const T* gb = dO + un.tok0 * (int64_t)g.d + un.head * HD;
    T* db = dqkv + un.tok0 * rs + un.head * HD;
    const LaneOff lq = lane_off<NC>(g.W, (uint32_t)rs, lr, gq), lg = lane_off<NC>(g.W, (uint32_t)g.d, lr, gq);
    uint32_t mw[2][3];
#pragma unroll
    for (int qh = 0; qh < 2; ++qh)
#pragma unroll
        for (int t = 0; t < 3; ++t) mw[qh][t] = maskrows[(un.w * 32 + 16 * qh + lr) * 3 + t];
    const uint32_t thresh = drop_thresh(ad.p);
    const float dscale = 1.0f / (1.0f - ad.p);
    const uint64_t TW = (uint64_t)g.F * g.W;
    const int fend = min(un.f1, g.F - 1);                        // last query frame that touches an owned key frame
    auto clampf = [&](int f) { return min(max(f, 0), g.F - 1); };

    struct KeyFrame { Rows<T, NC> k, v; Cols<T, NC> kc; };
    struct QFrame { Rows<T, NC> q, go; Cols<T, NC> qc, gc; };
    auto load_key = [&](int f) {
        KeyFrame x;
        x.k = load_rows<T, NC>(qb + f * fs + g.d, lq, 1.0f);
        x.v = load_rows<T, NC>(qb + f * fs + 2 * g.d, lq, 1.0f);
        x.kc = load_cols<T, NC>(qb + f * fs + g.d, lq, 1.0f);
        return x;
    };
    KeyFrame kw[3];
    kw[0] = load_key(clampf(un.f0 - 2));
    kw[1] = load_key(clampf(un.f0 - 1));
    f32x4v dk[3][2][NC], dv[3][2][NC];
#pragma unroll
    for (int t = 0; t < 3; ++t)
#pragma unroll
        for (int kh = 0; kh < 2; ++kh)
#pragma unroll
            for (int ct = 0; ct < NC; ++ct) { dk[t][kh][ct] = f32x4v{0.f, 0.f, 0.f, 0.f}; dv[t][kh][ct] = f32x4v{0.f, 0.f, 0.f, 0.f}; }

    QFrame nq;                                                   // one frame ahead: Q, dO of query frame f, key frame f + 1
    KeyFrame nk;
    auto fill = [&](int f) {
        const int fq = clampf(f);
        nq.q = load_rows<T, NC>(qb + fq * fs, lq, qmul);
        nq.qc = load_cols<T, NC>(qb + fq * fs, lq, qmul);
        nq.go = load_rows<T, NC>(gb + fq * gs, lg, 1.0f);
        nq.gc = load_cols<T, NC>(gb + fq * gs, lg, 1.0f);
        nk = load_key(clampf(f + 1));
    };
    if constexpr (PREF) fill(un.f0 - 1);

    auto store_key = [&](int f, const f32x4v (&k)[2][NC], const f32x4v (&v)[2][NC]) {
#pragma unroll
        for (int kh = 0; kh < 2; ++kh) {
            store_cols<T, NC>(db + f * fs + g.d, lq, kh, g.W, gq, k[kh], smul);
            store_cols<T, NC>(db + f * fs + 2 * g.d, lq, kh, g.W, gq, v[kh], 1.0f);
        }
    };

    for (int it = 0; it < g.seg + 2; ++it) {
        const int f = un.f0 - 1 + it;                            // query frame; slots t = 0, 1, 2 are key frames f-1, f, f+1
        __syncthreads();
        if constexpr (!PREF) fill(f);
        const QFrame q = nq;
        kw[2] = nk;
        if constexpr (PREF) fill(f + 1);
        if (f >= 0 && f <= fend && live) {
            const bool hp = f > 0, hn = f + 1 < g.F, own = f >= un.f0 && f < un.f1;
#pragma unroll
            for (int qh = 0; qh < 2; ++qh) {
                // ---- orientation 1: lane = query slot 16 qh + lr, registers = key slots 16 kh + 4g + r
                f32x4v s[3][2], p[3][2], ds[3][2];
                uint32_t nib[3][2];
                vis_nibbles(mw[qh], gq, hp, hn, nib);
#pragma unroll
                for (int t = 0; t < 3; ++t)
#pragma unroll
                    for (int kh = 0; kh < 2; ++kh) s[t][kh] = dot_rows<T, NC>(kw[t].k.c[kh], q.q.c[qh]) * smul;
                wband_softmax(s, nib, p);
                // attention dropout: A = D o P went into O = A V, so dP = D o dA (dA = dO V^T) and dV = A^T dO
                const uint64_t rowbase = (((uint64_t)un.bw * g.nH + un.head) * TW + (uint64_t)f * g.W + 16 * qh + lr) * TW;
                float delta = 0.f;
#pragma unroll
                for (int t = 0; t < 3; ++t)
#pragma unroll
                    for (int kh = 0; kh < 2; ++kh) {
                        f32x4v dp = dot_rows<T, NC>(kw[t].v.c[kh], q.go.c[qh]);              // dA[q = lr][key = 4g + r]
                        f32x4v a = p[t][kh];
                        if constexpr (ADROP) {
                            const f32x4v keep = wband_keep(ad.seed, rowbase, clampf(f - 1 + t), g.W, kh, gq, thresh, dscale);
                            dp *= keep;
                            a *= keep;
                        }
                        *reinterpret_cast<f32x4v*>(xs + ((t * 2 + kh) * 16 + lr) * XLD + 4 * gq) = a;
#pragma unroll
                        for (int r = 0; r < 4; ++r) delta += p[t][kh][r] * dp[r];
                        ds[t][kh] = dp;
                    }
                delta = xg_sum(delta);
                f32x4v acc[NC];
#pragma unroll
                for (int ct = 0; ct < NC; ++ct) acc[ct] = f32x4v{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int t = 0; t < 3; ++t)
#pragma unroll
                    for (int kh = 0; kh < 2; ++kh) {
                        ds[t][kh] = p[t][kh] * (ds[t][kh] - delta);
                        mul_cols<T, NC>(ds[t][kh], kw[t].kc.c[kh], acc);                     // dQ[q][c] = scale sum_key dS[q][key] K[key][c]
                    }
                if (own) store_cols<T, NC>(db + f * fs, lq, qh, g.W, gq, acc, band_scale<HD>());
                // ---- orientation 2: lane = key slot lr of tile (t, kh), registers = query slots 16 qh + 4g + r
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                __builtin_amdgcn_wave_barrier();
#pragma unroll
                for (int t = 0; t < 3; ++t)
#pragma unroll
                    for (int kh = 0; kh < 2; ++kh) {
                        f32x4v p2;
#pragma unroll
                        for (int r = 0; r < 4; ++r) p2[r] = xs[((t * 2 + kh) * 16 + 4 * gq + r) * XLD + lr];
                        mul_cols<T, NC>(p2, q.gc.c[qh], dv[t][kh]);                          // dV[key][c] += sum_q A[q][key] dO[q][c]
                    }
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                __builtin_amdgcn_wave_barrier();
#pragma unroll
                for (int t = 0; t < 3; ++t)
#pragma unroll
                    for (int kh = 0; kh < 2; ++kh)
                        *reinterpret_cast<f32x4v*>(xs + ((t * 2 + kh) * 16 + lr) * XLD + 4 * gq) = ds[t][kh];
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                __builtin_amdgcn_wave_barrier();
#pragma unroll
                for (int t = 0; t < 3; ++t)
#pragma unroll
                    for (int kh = 0; kh < 2; ++kh) {
                        f32x4v ds2;
#pragma unroll
                        for (int r = 0; r < 4; ++r) ds2[r] = xs[((t * 2 + kh) * 16 + 4 * gq + r) * XLD + lr];
                        mul_cols<T, NC>(ds2, q.qc.c[qh], dk[t][kh]);                         // dK[key][c] += sum_q dS[q][key] (scale Q)[q][c]
                    }
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                __builtin_amdgcn_wave_barrier();
            }
            // key frame f-1 has now seen query frames f-2, f-1, f; the clip's last key frame has no query frame f+1
            if (f - 1 >= un.f0) store_key(f - 1, dk[0], dv[0]);
            if (!hn && own) store_key(f, dk[1], dv[1]);
        }
#pragma unroll
        for (int kh = 0; kh < 2; ++kh)
#pragma unroll
            for (int ct = 0; ct < NC; ++ct) {
                dk[0][kh][ct] = dk[1][kh][ct]; dk[1][kh][ct] = dk[2][kh][ct]; dk[2][kh][ct] = f32x4v{0.f, 0.f, 0.f, 0.f};
                dv[0][kh][ct] = dv[1][kh][ct]; dv[1][kh][ct] = dv[2][kh][ct]; dv[2][kh][ct] = f32x4v{0.f, 0.f, 0.f, 0.f};
            }
        kw[0] = kw[1]; kw[1] = kw[2];
    }
}

bool wband_ok(int B, int F, int nW, int W, int nH, int hd) {
    return B > 0 && F > 0 && nW > 0 && W >= 1 && W <= 32 && nH > 0 && (hd == 16 || hd == 32) &&
           (int64_t)nW * W * 3 * nH * hd * 32 < 0x7fffffffLL;   // per-lane 32-bit offsets inside a frame
}

// enough wavefronts to fill the chip (256 CUs x 4 SIMDs x 2): cut the clip into frame segments of at least 8 frames
WGeom wband_geom(int B, int F, int nW, int W, int nH, int hd) {
    const int64_t base_units = (int64_t)B * nW * nH;
    int n_seg = 1;
    while (base_units * n_seg < 256 * 8 && F / (n_seg * 2) >= 8) n_seg *= 2;
    const int seg = (F + n_seg - 1) / n_seg;
    n_seg = (F + seg - 1) / seg;
    return WGeom{F, nW * W, W, nW, nH, nH * hd, seg, n_seg};
}

}  // namespace

extern "C" int hwgat_wband_attn_fwd_drop(const void* qkv, void* o, const uint32_t* maskrows, int B, int F, int nW, int W,
                                         int nH, int hd, int dtype, uint32_t drop_seed, float drop_p,
                                         const uint32_t* seed_base, void* stream) {
    if (!qkv || !o || !maskrows || !(drop_p >= 0.f) || drop_p >= 1.f) return HWGAT_EINVAL;
    if (!wband_ok(B, F, nW, W, nH, hd)) return HWGAT_ESHAPE;
    if (dtype != HWGAT_F32 && dtype != HWGAT_BF16) return HWGAT_EDTYPE;
    const AttnDrop ad = make_drop(drop_seed, drop_p, seed_base);
    const WGeom g = wband_geom(B, F, nW, W, nH, hd);
    const int64_t units = (int64_t)B * nW * nH * g.n_seg;
    if (units > 0x7fffffff) return HWGAT_ESHAPE;
    hipStream_t st = (hipStream_t)stream;
    const int blocks = (int)((units + 3) / 4);
#define FWD_ARGS(T) (const T*)qkv, (T*)o, maskrows, g, (int)units, ad
#define FWD(T)                                                                                   \
    if (ad.p > 0.f) {                                                                            \
        if (hd == 32) wband_attn_fwd_k<T, 32, 1, true><<<blocks, 256, 0, st>>>(FWD_ARGS(T));     \
        else wband_attn_fwd_k<T, 16, 2, true><<<blocks, 256, 0, st>>>(FWD_ARGS(T));              \
    } else if (hd == 32) wband_attn_fwd_k<T, 32, 1, false><<<blocks, 256, 0, st>>>(FWD_ARGS(T)); \
    else wband_attn_fwd_k<T, 16, 2, false><<<blocks, 256, 0, st>>>(FWD_ARGS(T));
    if (dtype == HWGAT_F32) { FWD(float) } else { FWD(bf16_t) }
#undef FWD
#undef FWD_ARGS
    HWGAT_LAUNCH_CHECK();
}

extern "C" int hwgat_wband_attn_fwd(const void* qkv, void* o, const uint32_t* maskrows, int B, int F, int nW, int W,
                                    int nH, int hd, int dtype, void* stream) {
    return hwgat_wband_attn_fwd_drop(qkv, o, maskrows, B, F, nW, W, nH, hd, dtype, 0u, 0.f, nullptr, stream);
}

extern "C" int hwgat_wband_attn_bwd_drop(const void* qkv, const void* dO, void* dqkv, const uint32_t* maskrows, int B,
                                         int F, int nW, int W, int nH, int hd, int dtype, uint32_t drop_seed,
                                         float drop_p, const uint32_t* seed_base, void* stream) {
    if (!qkv || !dO || !dqkv || !maskrows || !(drop_p >= 0.f) || drop_p >= 1.f) return HWGAT_EINVAL;
    if (!wband_ok(B, F, nW, W, nH, hd)) return HWGAT_ESHAPE;
    if (dtype != HWGAT_F32 && dtype != HWGAT_BF16) return HWGAT_EDTYPE;
    const AttnDrop ad = make_drop(drop_seed, drop_p, seed_base);
    const WGeom g = wband_geom(B, F, nW, W, nH, hd);
    const int64_t units = (int64_t)B * nW * nH * g.n_seg;
    if (units > 0x7fffffff) return HWGAT_ESHAPE;
    hipStream_t st = (hipStream_t)stream;
    const int blocks = (int)((units + 3) / 4);
#define BWD_ARGS(T) (const T*)qkv, (const T*)dO, (T*)dqkv, maskrows, g, (int)units, ad
#define BWD(T)                                                                                   \
    if (ad.p > 0.f) {                                                                            \
        if (hd == 32) wband_attn_bwd_k<T, 32, 1, true><<<blocks, 256, 0, st>>>(BWD_ARGS(T));     \
        else wband_attn_bwd_k<T, 16, 1, true><<<blocks, 256, 0, st>>>(BWD_ARGS(T));              \
    } else if (hd == 32) wband_attn_bwd_k<T, 32, 1, false><<<blocks, 256, 0, st>>>(BWD_ARGS(T)); \
    else wband_attn_bwd_k<T, 16, 1, false><<<blocks, 256, 0, st>>>(BWD_ARGS(T));
    if (dtype == HWGAT_F32) { BWD(float) } else { BWD(bf16_t) }
#undef BWD
#undef BWD_ARGS
    HWGAT_LAUNCH_CHECK();
}

extern "C" int hwgat_wband_attn_bwd(const void* qkv, const void* dO, void* dqkv, const uint32_t* maskrows, int B, int F,
                                    int nW, int W, int nH, int hd, int dtype, void* stream) {
    return hwgat_wband_attn_bwd_drop(qkv, dO, dqkv, maskrows, B, F, nW, W, nH, hd, dtype, 0u, 0.f, nullptr, stream);
}
