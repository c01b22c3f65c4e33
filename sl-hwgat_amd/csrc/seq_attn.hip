// Dense multi-head attention over the T <= 512 frames of a clip, head_dim 64, with a key-padding mask (the Transformer
// baseline, reference hwgat/models/Transformer.py: nn.MultiheadAttention(batch_first=True) with key_padding_mask).
//
// Layouts: qkv (B, T, 3d) as the in_proj linear writes it (q | k | v, head h at columns h*64 .. h*64+63 of each third),
// o (B, T, d) as out_proj reads it, dqkv like qkv.  pad: (B, nw) uint32 words, nw = ceil(T / 32); bit t of clip b set =
// frame t is padding (made on the device by hwgat_seq_embed_fwd).  lse / D: (B, nH, T) fp32 row statistics.
//
// Padding rule (torch 2.10): a padded key gets probability 0; a query whose keys are ALL padded gets o = 0 and no
// gradient (its lse is -inf and every key is skipped).  Attention dropout: keep(i, j) is the common hash of
// (site seed + *seed_base, ((b nH + h) T + i) T + j), so hwgat_dropout_mask_f32 reproduces the (B, nH, T, T) mask.
//
// Work split: one thread owns one query (forward) or one half of a query / key row (backward: 32 of the 64 dims, the
// pair partner holds the other half and dot products are completed with one DPP exchange).  Keys (forward, dQ) or
// queries (dK / dV) stream through LDS in tiles of 64 rows, broadcast to every thread; the softmax is online in the
// forward (m, l per query) and recomputed from lse in the backward.  The backward is two launches: dQ (+ D = dO . o)
// per query tile, then dK, dV per key tile; every output element has exactly one writer, so there are no atomics and
// the result is bit-reproducible.  Arithmetic is fp32 FMA for both activation dtypes (bf16 is converted on load).
#include "common.h"
#include "fused_ops.h"

namespace {

constexpr int HD = 64;          // head_dim
constexpr int TILE = 64;        // rows per LDS tile
constexpr float QSCALE = 0.125f;  // 64 ** -0.5

struct SeqArgs {
    const void* qkv; const void* o; const void* dout; void* out; void* dqkv;
    const uint32_t* pad; float* lse; float* D;
    int B, T, nH, nw;
    uint32_t seed; float p; const uint32_t* seed_base;
};

template <typename T> __device__ __forceinline__ float ldf(const T* p) { return (float)*p; }
template <typename T> __device__ __forceinline__ void load_row(const T* src, float* dst, int n) {
    for (int e = 0; e < n; e += 4) {
        float v[4];
        io<T>::load4(src + e, v);
        dst[e] = v[0]; dst[e + 1] = v[1]; dst[e + 2] = v[2]; dst[e + 3] = v[3];
    }
}

__device__ __forceinline__ bool is_pad(const uint32_t* pad, int nw, int b, int t) {
    return (pad[(int64_t)b * nw + (t >> 5)] >> (t & 31)) & 1u;
}

// sum of a value over the lane pair (2k, 2k+1): DPP quad_perm [1,0,3,2]
__device__ __forceinline__ float pair_sum(float v) {
    return v + __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0xB1, 0xf, 0xf, true));
}

// stage rows [r0, r0 + TILE) of one 64-wide column block of a (B, T, ld) tensor into LDS as fp32 (rows >= T -> 0)
template <typename T>
__device__ __forceinline__ void stage(float (*dst)[HD + 4], const T* base, int ld, int r0, int Tn, int nthreads) {
    for (int q = threadIdx.x; q < TILE * (HD / 4); q += nthreads) {
        const int r = q / (HD / 4), c = (q % (HD / 4)) * 4;
        float v[4] = {0.f, 0.f, 0.f, 0.f};
        if (r0 + r < Tn) io<T>::load4(base + (int64_t)(r0 + r) * ld + c, v);
        dst[r][c] = v[0]; dst[r][c + 1] = v[1]; dst[r][c + 2] = v[2]; dst[r][c + 3] = v[3];
    }
}

// fp32: two waves per workgroup share one K / V tile in LDS, so that the 35 KB of LDS hold two waves per SIMD, not one
constexpr int FQ = 128;         // queries per forward workgroup (fp32)
constexpr int BQ = 128;         // rows per backward workgroup (fp32; 256 threads, a lane pair per row)

// ---------------------------------------------------------------- forward: FQ threads, one query each
template <typename T, bool DROP>
__global__ __launch_bounds__(FQ) void seq_attn_fwd_k(SeqArgs a) {
    __shared__ float ks[TILE][HD + 4], vs[TILE][HD + 4];
    __shared__ uint32_t kpad[TILE];
    const int b = blockIdx.z, h = blockIdx.y, i = blockIdx.x * FQ + threadIdx.x;
    const int d = a.nH * HD, ld = 3 * d;
    const T* qkv = (const T*)a.qkv + (int64_t)b * a.T * ld;
    const uint32_t seed = a.seed + seed_base_of(a.seed_base);
    const uint32_t th = drop_thresh(a.p);
    const float dsc = 1.0f / (1.0f - a.p);
    float q[HD], acc[HD];
    if (i < a.T) load_row(qkv + (int64_t)i * ld + h * HD, q, HD);
    else for (int e = 0; e < HD; ++e) q[e] = 0.f;
#pragma unroll
    for (int e = 0; e < HD; ++e) { q[e] *= QSCALE; acc[e] = 0.f; }
    float m = -INFINITY, l = 0.f;
    const uint64_t drow = (((uint64_t)b * a.nH + h) * a.T + (uint64_t)i) * a.T;
    for (int j0 = 0; j0 < a.T; j0 += TILE) {
        __syncthreads();
        stage<T>(ks, qkv + d + h * HD, ld, j0, a.T, FQ);
        stage<T>(vs, qkv + 2 * d + h * HD, ld, j0, a.T, FQ);
        if (threadIdx.x < TILE) kpad[threadIdx.x] = (j0 + threadIdx.x >= a.T) || is_pad(a.pad, a.nw, b, j0 + threadIdx.x);
        __syncthreads();
        const int nj = min(TILE, a.T - j0);
        for (int jj = 0; jj < nj; ++jj) {
            if (kpad[jj]) continue;
            float s = 0.f;
#pragma unroll
            for (int e = 0; e < HD; ++e) s = fmaf(q[e], ks[jj][e], s);
            const float mn = fmaxf(m, s);
            const float corr = __expf(m - mn);          // m = -inf on the first visible key: corr = 0
            const float pe = __expf(s - mn);
            l = l * corr + pe;
            float w = pe;
            if constexpr (DROP) w *= drop_keep(seed, drow + (uint64_t)(j0 + jj), th, dsc);
#pragma unroll
            for (int e = 0; e < HD; ++e) acc[e] = fmaf(w, vs[jj][e], acc[e] * corr);
            m = mn;
        }
    }
    if (i >= a.T) return;
    const float inv = l > 0.f ? 1.0f / l : 0.f;       // every key padded: o = 0
    T* out = (T*)a.out + ((int64_t)b * a.T + i) * d + h * HD;
    for (int e = 0; e < HD; e += 4) {
        const float v[4] = {acc[e] * inv, acc[e + 1] * inv, acc[e + 2] * inv, acc[e + 3] * inv};
        io<T>::store4(out + e, v);
    }
    if (a.lse) a.lse[((int64_t)b * a.nH + h) * a.T + i] = l > 0.f ? m + __logf(l) : -INFINITY;
}

// ---------------------------------------------------------------- backward, dQ: 2 BQ threads, a lane pair per query
template <typename T, bool DROP>
__global__ __launch_bounds__(2 * BQ) void seq_attn_bwd_dq_k(SeqArgs a) {
    __shared__ float ks[TILE][HD + 4], vs[TILE][HD + 4];
    __shared__ uint32_t kpad[TILE];
    constexpr int H2 = HD / 2;
    const int b = blockIdx.z, h = blockIdx.y, i = blockIdx.x * BQ + threadIdx.x / 2, half = threadIdx.x & 1;
    const int d = a.nH * HD, ld = 3 * d;
    const T* qkv = (const T*)a.qkv + (int64_t)b * a.T * ld;
    const uint32_t seed = a.seed + seed_base_of(a.seed_base);
    const uint32_t th = drop_thresh(a.p);
    const float dsc = 1.0f / (1.0f - a.p);
    const bool live = i < a.T;
    const int64_t row = (int64_t)b * a.T + (live ? i : 0);
    const int c0 = h * HD + half * H2;
    float q[H2], dO[H2], dq[H2];
    float Dp = 0.f;
    if (live) {
        float o[H2];
        load_row(qkv + (int64_t)i * ld + c0, q, H2);
        load_row((const T*)a.dout + row * d + c0, dO, H2);
        load_row((const T*)a.o + row * d + c0, o, H2);
#pragma unroll
        for (int e = 0; e < H2; ++e) Dp = fmaf(dO[e], o[e], Dp);
    } else {
        for (int e = 0; e < H2; ++e) q[e] = dO[e] = 0.f;
    }
    const float D = pair_sum(Dp);
    const int64_t si = ((int64_t)b * a.nH + h) * a.T + (live ? i : 0);
    const float lse = live ? a.lse[si] : -INFINITY;
#pragma unroll
    for (int e = 0; e < H2; ++e) { q[e] *= QSCALE; dq[e] = 0.f; }
    const uint64_t drow = (((uint64_t)b * a.nH + h) * a.T + (uint64_t)i) * a.T;
    for (int j0 = 0; j0 < a.T; j0 += TILE) {
        __syncthreads();
        stage<T>(ks, qkv + d + h * HD, ld, j0, a.T, 2 * BQ);
        stage<T>(vs, qkv + 2 * d + h * HD, ld, j0, a.T, 2 * BQ);
        if (threadIdx.x < TILE) kpad[threadIdx.x] = (j0 + threadIdx.x >= a.T) || is_pad(a.pad, a.nw, b, j0 + threadIdx.x);
        __syncthreads();
        const int nj = min(TILE, a.T - j0);
        for (int jj = 0; jj < nj; ++jj) {
            if (kpad[jj]) continue;                     // uniform over the block
            float s = 0.f, dp = 0.f;
#pragma unroll
            for (int e = 0; e < H2; ++e) {
                s = fmaf(q[e], ks[jj][half * H2 + e], s);
                dp = fmaf(dO[e], vs[jj][half * H2 + e], dp);
            }
            s = pair_sum(s);
            dp = pair_sum(dp);
            const float pr = live ? __expf(s - lse) : 0.f;
            if constexpr (DROP) dp *= drop_keep(seed, drow + (uint64_t)(j0 + jj), th, dsc);
            const float ds = pr * (dp - D) * QSCALE;
#pragma unroll
            for (int e = 0; e < H2; ++e) dq[e] = fmaf(ds, ks[jj][half * H2 + e], dq[e]);
        }
    }
    if (!live) return;
    T* dst = (T*)a.dqkv + (int64_t)row * ld + c0;
    for (int e = 0; e < H2; e += 4) {
        const float v[4] = {dq[e], dq[e + 1], dq[e + 2], dq[e + 3]};
        io<T>::store4(dst + e, v);
    }
    if (half == 0) a.D[si] = D;
}

// ---------------------------------------------------------------- backward, dK / dV: 2 BQ threads, a lane pair per key
template <typename T, bool DROP>
__global__ __launch_bounds__(2 * BQ) void seq_attn_bwd_dkv_k(SeqArgs a) {
    __shared__ float qs[TILE][HD + 4], os[TILE][HD + 4];
    __shared__ float ql[TILE], qd[TILE];
    constexpr int H2 = HD / 2;
    const int b = blockIdx.z, h = blockIdx.y, j = blockIdx.x * BQ + threadIdx.x / 2, half = threadIdx.x & 1;
    const int d = a.nH * HD, ld = 3 * d;
    const T* qkv = (const T*)a.qkv + (int64_t)b * a.T * ld;
    const T* dout = (const T*)a.dout + (int64_t)b * a.T * d;
    const uint32_t seed = a.seed + seed_base_of(a.seed_base);
    const uint32_t th = drop_thresh(a.p);
    const float dsc = 1.0f / (1.0f - a.p);
    const bool live = j < a.T && !is_pad(a.pad, a.nw, b, j < a.T ? j : 0);
    const int c0 = h * HD + half * H2;
    float k[H2], v[H2], dk[H2], dv[H2];
    if (live) {
        load_row(qkv + (int64_t)j * ld + d + c0, k, H2);
        load_row(qkv + (int64_t)j * ld + 2 * d + c0, v, H2);
    } else {
        for (int e = 0; e < H2; ++e) k[e] = v[e] = 0.f;
    }
#pragma unroll
    for (int e = 0; e < H2; ++e) { dk[e] = 0.f; dv[e] = 0.f; }
    const int64_t s0 = ((int64_t)b * a.nH + h) * a.T;
    for (int i0 = 0; i0 < a.T; i0 += TILE) {
        __syncthreads();
        stage<T>(qs, qkv + h * HD, ld, i0, a.T, 2 * BQ);
        stage<T>(os, dout + h * HD, d, i0, a.T, 2 * BQ);
        if (threadIdx.x < TILE) {
            const int ii = i0 + threadIdx.x;
            ql[threadIdx.x] = ii < a.T ? a.lse[s0 + ii] : -INFINITY;
            qd[threadIdx.x] = ii < a.T ? a.D[s0 + ii] : 0.f;
        }
        __syncthreads();
        const int ni = min(TILE, a.T - i0);
        for (int ii = 0; ii < ni; ++ii) {
            float s = 0.f, dp = 0.f;
#pragma unroll
            for (int e = 0; e < H2; ++e) {
                s = fmaf(qs[ii][half * H2 + e], k[e], s);
                dp = fmaf(os[ii][half * H2 + e], v[e], dp);
            }
            s = pair_sum(s) * QSCALE;
            dp = pair_sum(dp);
            // a padded key (live = false) and a query without any visible key (lse = -inf) contribute nothing
            const float pr = (live && ql[ii] != -INFINITY) ? __expf(s - ql[ii]) : 0.f;
            float z = 1.f;
            if constexpr (DROP) z = drop_keep(seed, ((uint64_t)s0 + (uint64_t)(i0 + ii)) * a.T + (uint64_t)j, th, dsc);
            const float pz = pr * z;
            const float ds = pr * (dp * z - qd[ii]) * QSCALE;
#pragma unroll
            for (int e = 0; e < H2; ++e) {
                dv[e] = fmaf(pz, os[ii][half * H2 + e], dv[e]);
                dk[e] = fmaf(ds, qs[ii][half * H2 + e], dk[e]);
            }
        }
    }
    if (j >= a.T) return;
    T* dst = (T*)a.dqkv + ((int64_t)b * a.T + j) * ld;
    for (int e = 0; e < H2; e += 4) {
        const float kv[4] = {dk[e], dk[e + 1], dk[e + 2], dk[e + 3]};
        const float vv[4] = {dv[e], dv[e + 1], dv[e + 2], dv[e + 3]};
        io<T>::store4(dst + d + c0 + e, kv);
        io<T>::store4(dst + 2 * d + c0 + e, vv);
    }
}

// ---------------------------------------------------------------- bf16: the same three passes on v_mfma_f32_32x32x16_bf16
// One wave per workgroup, 32 rows of the tile dimension on the MFMA lanes (r = lane & 31, lane half hh = lane >> 5).
// Operand maps (gfx950): A[row r][k = 8 hh + j], B[k = 8 hh + j][col r] for element j of a k-step of 16; accumulator
// element i of lane (r, hh) is C[row crow(i, hh)][col r].  Products whose k runs over 64 head dims take both operands as
// contiguous 16-byte row pieces straight from memory.  Products whose k runs over the 32 keys (or queries) of a tile take
// the previous accumulator as the B operand (registers 8s .. 8s+7 -> k-step s, k order 16 s + 8 (j >> 2) + 4 hh + (j & 3))
// and the other operand from a transposed LDS image of the tile.  Scores and probabilities are fp32; they are rounded to
// bf16 only as the operand of the second product, as flash attention does.
typedef float f32x16v __attribute__((ext_vector_type(16)));
constexpr int MT = 32;                  // rows per MFMA tile

__device__ __forceinline__ f32x16v mfma32(bf16x8 a, bf16x8 b, f32x16v c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ bf16x8 ld8(const bf16_t* p, bool ok) {
    if (ok) return *reinterpret_cast<const bf16x8*>(p);
    bf16x8 z;
#pragma unroll
    for (int j = 0; j < 8; ++j) z[j] = (bf16_t)0.f;
    return z;
}
// registers 8s .. 8s+7 of an accumulator as the bf16 B operand of k-step s
__device__ __forceinline__ bf16x8 pack_k(const f32x16v& v, int s) {
    bf16x8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = (bf16_t)v[8 * s + j];
    return o;
}
// the A operand paired with pack_k: element j = img[row][16 s + 8 (j >> 2) + 4 hh + (j & 3)] of a [row][tile index] image
__device__ __forceinline__ bf16x8 gather_k(const bf16_t* row, int s, int hh) {
    bf16x8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = row[16 * s + 8 * (j >> 2) + 4 * hh + (j & 3)];
    return o;
}
constexpr int TLD = MT + 8;             // row stride of the transposed tile images (elements)
// transposed image img[dim][t] of rows base[t0 + t][0 .. 63] (t < 32): lane (r, hh) moves row r, dims 32 hh .. 32 hh + 31
__device__ __forceinline__ void stage_t(bf16_t (*img)[TLD], const bf16_t* base, int ld, int t0, int Tn, int r, int hh) {
    const bool ok = t0 + r < Tn;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const bf16x8 v = ld8(base + (int64_t)(t0 + r) * ld + 32 * hh + 8 * c, ok);
#pragma unroll
        for (int j = 0; j < 8; ++j) img[32 * hh + 8 * c + j][r] = v[j];
    }
}

template <bool DROP>
__global__ __launch_bounds__(64) void seq_attn_fwd_mfma_k(SeqArgs a) {
    __shared__ bf16_t vt[HD][TLD];
    const int lane = threadIdx.x, r = lane & 31, hh = lane >> 5;
    const int b = blockIdx.z, h = blockIdx.y, q = blockIdx.x * MT + r;
    const int d = a.nH * HD, ld = 3 * d;
    const bf16_t* qkv = (const bf16_t*)a.qkv + (int64_t)b * a.T * ld;
    const uint32_t seed = a.seed + seed_base_of(a.seed_base);
    const uint32_t th = drop_thresh(a.p);
    const float dsc = 1.0f / (1.0f - a.p);
    const bool qv = q < a.T;
    bf16x8 qf[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) qf[s] = ld8(qkv + (int64_t)q * ld + h * HD + 16 * s + 8 * hh, qv);
    f32x16v o0 = {}, o1 = {};
    float m = -INFINITY, l = 0.f;
    const uint64_t drow = (((uint64_t)b * a.nH + h) * a.T + (uint64_t)q) * a.T;
    for (int j0 = 0; j0 < a.T; j0 += MT) {
        const int key = j0 + r;
        f32x16v st = {};                                    // S^T: row = key, col = query
#pragma unroll
        for (int s = 0; s < 4; ++s) st = mfma32(ld8(qkv + (int64_t)key * ld + d + h * HD + 16 * s + 8 * hh, key < a.T), qf[s], st);
        __syncthreads();
        stage_t(vt, qkv + 2 * d + h * HD, ld, j0, a.T, r, hh);
        __syncthreads();
        float tmax = -INFINITY;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int kk = j0 + crow(i, hh);
            const bool masked = kk >= a.T || is_pad(a.pad, a.nw, b, kk);
            st[i] = masked ? -INFINITY : st[i] * QSCALE;
            tmax = fmaxf(tmax, st[i]);
        }
        tmax = fmaxf(tmax, __shfl_xor(tmax, 32, 64));
        const float mn = fmaxf(m, tmax);
        const float corr = mn == -INFINITY ? 1.f : __expf(m - mn);
        float ls = 0.f;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            float pe = st[i] == -INFINITY ? 0.f : __expf(st[i] - mn);
            ls += pe;
            if constexpr (DROP) pe *= drop_keep(seed, drow + (uint64_t)(j0 + crow(i, hh)), th, dsc);
            st[i] = pe;
        }
        ls += __shfl_xor(ls, 32, 64);
        l = l * corr + ls;
        m = mn;
        o0 *= corr;
        o1 *= corr;
#pragma unroll
        for (int s = 0; s < 2; ++s) {                       // O^T += V^T P^T: row = dim, col = query
            const bf16x8 pb = pack_k(st, s);
            o0 = mfma32(gather_k(vt[r], s, hh), pb, o0);
            o1 = mfma32(gather_k(vt[32 + r], s, hh), pb, o1);
        }
    }
    if (!qv) return;
    const float inv = l > 0.f ? 1.0f / l : 0.f;             // every key padded: o = 0
    bf16_t* out = (bf16_t*)a.out + ((int64_t)b * a.T + q) * d + h * HD;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        out[crow(i, hh)] = (bf16_t)(o0[i] * inv);
        out[32 + crow(i, hh)] = (bf16_t)(o1[i] * inv);
    }
    if (a.lse && hh == 0) a.lse[((int64_t)b * a.nH + h) * a.T + q] = l > 0.f ? m + __logf(l) : -INFINITY;
}

template <bool DROP>
__global__ __launch_bounds__(64) void seq_attn_bwd_dq_mfma_k(SeqArgs a) {
    __shared__ bf16_t kt[HD][TLD];
    const int lane = threadIdx.x, r = lane & 31, hh = lane >> 5;
    const int b = blockIdx.z, h = blockIdx.y, q = blockIdx.x * MT + r;
    const int d = a.nH * HD, ld = 3 * d;
    const bf16_t* qkv = (const bf16_t*)a.qkv + (int64_t)b * a.T * ld;
    const uint32_t seed = a.seed + seed_base_of(a.seed_base);
    const uint32_t th = drop_thresh(a.p);
    const float dsc = 1.0f / (1.0f - a.p);
    const bool qv = q < a.T;
    const int64_t row = (int64_t)b * a.T + (qv ? q : 0);
    const bf16_t* dO = (const bf16_t*)a.dout + row * d + h * HD;
    const bf16_t* oo = (const bf16_t*)a.o + row * d + h * HD;
    bf16x8 qf[4], df[4];
    float Dp = 0.f;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        qf[s] = ld8(qkv + (int64_t)q * ld + h * HD + 16 * s + 8 * hh, qv);
        df[s] = ld8(dO + 16 * s + 8 * hh, qv);
        const bf16x8 ov = ld8(oo + 16 * s + 8 * hh, qv);
#pragma unroll
        for (int j = 0; j < 8; ++j) Dp = fmaf((float)df[s][j], (float)ov[j], Dp);
    }
    const float D = Dp + __shfl_xor(Dp, 32, 64);
    const int64_t si = ((int64_t)b * a.nH + h) * a.T + (qv ? q : 0);
    const float lse = qv ? a.lse[si] : -INFINITY;
    f32x16v g0 = {}, g1 = {};                                // dQ^T: row = dim, col = query
    const uint64_t drow = (((uint64_t)b * a.nH + h) * a.T + (uint64_t)q) * a.T;
    for (int j0 = 0; j0 < a.T; j0 += MT) {
        const int key = j0 + r;
        f32x16v st = {}, dpt = {};                          // S^T, dP^T: row = key, col = query
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            st = mfma32(ld8(qkv + (int64_t)key * ld + d + h * HD + 16 * s + 8 * hh, key < a.T), qf[s], st);
            dpt = mfma32(ld8(qkv + (int64_t)key * ld + 2 * d + h * HD + 16 * s + 8 * hh, key < a.T), df[s], dpt);
        }
        __syncthreads();
        stage_t(kt, qkv + d + h * HD, ld, j0, a.T, r, hh);
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int kk = j0 + crow(i, hh);
            const bool masked = kk >= a.T || is_pad(a.pad, a.nw, b, kk) || lse == -INFINITY;
            const float pr = masked ? 0.f : __expf(st[i] * QSCALE - lse);
            float dp = dpt[i];
            if constexpr (DROP) dp *= drop_keep(seed, drow + (uint64_t)kk, th, dsc);
            st[i] = pr * (dp - D) * QSCALE;
        }
#pragma unroll
        for (int s = 0; s < 2; ++s) {                       // dQ^T += K^T dS^T
            const bf16x8 sb = pack_k(st, s);
            g0 = mfma32(gather_k(kt[r], s, hh), sb, g0);
            g1 = mfma32(gather_k(kt[32 + r], s, hh), sb, g1);
        }
    }
    if (!qv) return;
    bf16_t* dst = (bf16_t*)a.dqkv + row * ld + h * HD;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        dst[crow(i, hh)] = (bf16_t)g0[i];
        dst[32 + crow(i, hh)] = (bf16_t)g1[i];
    }
    if (hh == 0) a.D[si] = D;
}

template <bool DROP>
__global__ __launch_bounds__(64) void seq_attn_bwd_dkv_mfma_k(SeqArgs a) {
    __shared__ bf16_t qt[HD][TLD], dt[HD][TLD];
    __shared__ float qls[MT], qdd[MT];
    const int lane = threadIdx.x, r = lane & 31, hh = lane >> 5;
    const int b = blockIdx.z, h = blockIdx.y, key = blockIdx.x * MT + r;
    const int d = a.nH * HD, ld = 3 * d;
    const bf16_t* qkv = (const bf16_t*)a.qkv + (int64_t)b * a.T * ld;
    const bf16_t* dout = (const bf16_t*)a.dout + (int64_t)b * a.T * d;
    const uint32_t seed = a.seed + seed_base_of(a.seed_base);
    const uint32_t th = drop_thresh(a.p);
    const float dsc = 1.0f / (1.0f - a.p);
    const bool kin = key < a.T;
    const bool live = kin && !is_pad(a.pad, a.nw, b, kin ? key : 0);
    bf16x8 kf[4], vf[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        kf[s] = ld8(qkv + (int64_t)key * ld + d + h * HD + 16 * s + 8 * hh, kin);
        vf[s] = ld8(qkv + (int64_t)key * ld + 2 * d + h * HD + 16 * s + 8 * hh, kin);
    }
    f32x16v k0 = {}, k1 = {}, v0 = {}, v1 = {};              // dK^T, dV^T: row = dim, col = key
    const int64_t s0 = ((int64_t)b * a.nH + h) * a.T;
    for (int i0 = 0; i0 < a.T; i0 += MT) {
        const int qrow = i0 + r;
        const bool qv = qrow < a.T;
        f32x16v sc = {}, dp = {};                           // S, dP: row = query, col = key
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            sc = mfma32(ld8(qkv + (int64_t)qrow * ld + h * HD + 16 * s + 8 * hh, qv), kf[s], sc);
            dp = mfma32(ld8(dout + (int64_t)qrow * d + h * HD + 16 * s + 8 * hh, qv), vf[s], dp);
        }
        __syncthreads();
        stage_t(qt, qkv + h * HD, ld, i0, a.T, r, hh);
        stage_t(dt, dout + h * HD, d, i0, a.T, r, hh);
        if (hh == 0) {
            qls[r] = qv ? a.lse[s0 + qrow] : -INFINITY;
            qdd[r] = qv ? a.D[s0 + qrow] : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int qi = crow(i, hh);
            const float lq = qls[qi];
            // a padded key, a query past T and a query without any visible key contribute nothing
            const float pr = (live && lq != -INFINITY) ? __expf(sc[i] * QSCALE - lq) : 0.f;
            float z = 1.f;
            if constexpr (DROP) z = drop_keep(seed, ((uint64_t)s0 + (uint64_t)(i0 + qi)) * a.T + (uint64_t)key, th, dsc);
            sc[i] = pr * z;
            dp[i] = pr * (dp[i] * z - qdd[qi]) * QSCALE;
        }
#pragma unroll
        for (int s = 0; s < 2; ++s) {                       // dV^T += dO^T (P z), dK^T += Q^T dS
            const bf16x8 pb = pack_k(sc, s), sb = pack_k(dp, s);
            v0 = mfma32(gather_k(dt[r], s, hh), pb, v0);
            v1 = mfma32(gather_k(dt[32 + r], s, hh), pb, v1);
            k0 = mfma32(gather_k(qt[r], s, hh), sb, k0);
            k1 = mfma32(gather_k(qt[32 + r], s, hh), sb, k1);
        }
    }
    if (!kin) return;
    bf16_t* dst = (bf16_t*)a.dqkv + ((int64_t)b * a.T + key) * ld + h * HD;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        dst[d + crow(i, hh)] = (bf16_t)k0[i];
        dst[d + 32 + crow(i, hh)] = (bf16_t)k1[i];
        dst[2 * d + crow(i, hh)] = (bf16_t)v0[i];
        dst[2 * d + 32 + crow(i, hh)] = (bf16_t)v1[i];
    }
}

int check(int B, int T, int nH, int hd, int dtype) {
    if (B <= 0 || T <= 0 || nH <= 0) return HWGAT_EINVAL;
    if (hd != HD || T > 512 || B > 65535 || nH > 65535) return HWGAT_ESHAPE;
    if (dtype != HWGAT_F32 && dtype != HWGAT_BF16) return HWGAT_EDTYPE;
    return 0;
}

}  // namespace

extern "C" int hwgat_seq_attn_fwd(const void* qkv, void* o, float* lse, const uint32_t* pad, int B, int T, int n_heads,
                                  int head_dim, int dtype, uint32_t seed, float p, const uint32_t* seed_base, void* stream) {
    if (!qkv || !o || !pad) return HWGAT_EINVAL;
    if (const int rc = check(B, T, n_heads, head_dim, dtype)) return rc;
    if (p < 0.f || p >= 1.f) return HWGAT_EINVAL;
    SeqArgs a{qkv, nullptr, nullptr, o, nullptr, pad, lse, nullptr, B, T, n_heads, (T + 31) / 32, seed, p, seed_base};
    hipStream_t st = (hipStream_t)stream;
    const bool drop = p * 65536.0f + 0.5f >= 1.0f;     // drop_thresh(p) != 0
    if (dtype == HWGAT_F32) {
        const dim3 gf((T + FQ - 1) / FQ, n_heads, B);
        if (drop) seq_attn_fwd_k<float, true><<<gf, FQ, 0, st>>>(a);
        else seq_attn_fwd_k<float, false><<<gf, FQ, 0, st>>>(a);
    } else {
        const dim3 g32((T + MT - 1) / MT, n_heads, B);
        if (drop) seq_attn_fwd_mfma_k<true><<<g32, 64, 0, st>>>(a);
        else seq_attn_fwd_mfma_k<false><<<g32, 64, 0, st>>>(a);
    }
    HWGAT_LAUNCH_CHECK();
}

extern "C" int hwgat_seq_attn_bwd(const void* qkv, const void* o, const void* dout, const float* lse, const uint32_t* pad,
                                  void* dqkv, float* D, int B, int T, int n_heads, int head_dim, int dtype, uint32_t seed,
                                  float p, const uint32_t* seed_base, void* stream) {
    if (!qkv || !o || !dout || !lse || !pad || !dqkv || !D) return HWGAT_EINVAL;
    if (const int rc = check(B, T, n_heads, head_dim, dtype)) return rc;
    if (p < 0.f || p >= 1.f) return HWGAT_EINVAL;
    SeqArgs a{qkv, o, dout, nullptr, dqkv, pad, const_cast<float*>(lse), D, B, T, n_heads, (T + 31) / 32, seed, p, seed_base};
    const dim3 gb((T + BQ - 1) / BQ, n_heads, B);
    hipStream_t st = (hipStream_t)stream;
    const bool drop = p * 65536.0f + 0.5f >= 1.0f;     // drop_thresh(p) != 0
#define SEQ_BWD(TY, DR)                                               \
    do {                                                              \
        seq_attn_bwd_dq_k<TY, DR><<<gb, 2 * BQ, 0, st>>>(a);          \
        seq_attn_bwd_dkv_k<TY, DR><<<gb, 2 * BQ, 0, st>>>(a);         \
    } while (0)
    if (dtype == HWGAT_F32) {
        if (drop) SEQ_BWD(float, true); else SEQ_BWD(float, false);
    } else {
        const dim3 g32((T + MT - 1) / MT, n_heads, B);
        if (drop) {
            seq_attn_bwd_dq_mfma_k<true><<<g32, 64, 0, st>>>(a);
            seq_attn_bwd_dkv_mfma_k<true><<<g32, 64, 0, st>>>(a);
        } else {
            seq_attn_bwd_dq_mfma_k<false><<<g32, 64, 0, st>>>(a);
            seq_attn_bwd_dkv_mfma_k<false><<<g32, 64, 0, st>>>(a);
        }
    }
#undef SEQ_BWD
    HWGAT_LAUNCH_CHECK();
}
