// Smoothed cross-entropy on the classifier's logits and the device-side evaluation accumulators (reference:
// hwgat/losses/SmoothCrossEntropy.py, hwgat/utils.py:118-161 evaluate / predictions_plus_true, :324-350 gen_cm_w).
//
//   hwgat_sce_fwd          sce_fwd_k: one workgroup per row -- max / arg-max / sum z, then sum exp / rank count; the row is
//                          staged in LDS when it fits (C <= SCE_LDS_FLOATS), else read twice; 16-byte loads when
//                          C % 4 == 0.  sce_mean_k (one workgroup) then takes the mean of the row losses in a fixed order.
//   hwgat_sce_bwd          sce_bwd_k: one pass over the logits with the stored lse.
//   hwgat_eval_accumulate  eval_acc_k: one workgroup folds a batch into the accumulator block (layout: hwgat_hip.h).
//   hwgat_bsce_fwd         the loss of one SLICE of a padded batch (train.BatchSlicedCrossEntropyLoss): bsce_live_k turns
//                          the batch's row count and the slice's offset into the slice's live-row count, sce_fwd_k runs
//                          on those rows, bsce_sum_k (one workgroup) adds their losses in a fixed order, divides by the
//                          BATCH's row count and counts the live rows whose target ranks first.
//   hwgat_bsce_bwd         bsce_bwd_k: sce_bwd_k with the batch's row count as the divisor; exact zeros for the other rows.
//   hwgat_mbsce_fwd / _bwd the same slice with two targets and a weight per row (train.MixedCrossEntropyLoss): sce_fwd_k
//                          once per target, mbsce_sum_k blends the row losses and sums; mbsce_bwd_k is bsce_bwd_k with the
//                          one-hot replaced by lam [j == t] + (1 - lam) [j == t_b].
//   hwgat_kd_fwd / _bwd    the same slice with a teacher's logits beside the labels (train.DistilledCrossEntropyLoss):
//                          sce_fwd_k once per target as above, kd_row_k (one workgroup per row, both rows staged in LDS
//                          when C <= KD_LDS_FLOATS) the tempered KL of the row, kd_sum_k the blend and every sum;
//                          kd_bwd_k is mbsce_bwd_k plus the soft term.  alpha and tau are device words (hwgat_kd_set).
//
// No float or double atomic anywhere: every floating-point sum is a per-thread strided sum followed by a fixed butterfly
// and a fixed combination of the four waves, so every output is bit-reproducible.  The integer counters of the
// accumulator use integer atomicAdd (order does not change an integer sum).
// A target outside [0, C) is never used as an index: it is replaced by 0 for addressing and the row is marked bad.
#include "common.h"
#include <limits.h>
#include <math.h>

namespace {

constexpr int SCE_THREADS = 256;
constexpr int SCE_LDS_FLOATS = 8192;           // rows of up to 32 KB are staged in LDS
constexpr int SCE_MAX_C = 65536;

template <typename T>
__device__ __forceinline__ T wave_all_sum(T v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// sum over the workgroup's 256 threads in a fixed order; `red` holds 4 values and may be reused right after the call
template <typename T>
__device__ __forceinline__ T block_sum(T v, T* red) {
    v = wave_all_sum(v);
    __syncthreads();
    if (lane_id() == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

// rows that take part: *n_valid clamped to [0, B], all B when the pointer is NULL
__device__ __forceinline__ int64_t valid_rows(const int32_t* n_valid, int64_t B) {
    if (!n_valid) return B;
    const int64_t n = *n_valid;
    return n < 0 ? 0 : (n > B ? B : n);
}

__device__ __forceinline__ void take_max(float v, int j, float& m, int& mi) {
    if (v > m) { m = v; mi = j; }                // strict: the lowest index of equal values stays; a NaN never enters
}

template <bool STAGED, bool VEC>
__global__ __launch_bounds__(SCE_THREADS) void sce_fwd_k(const float* __restrict__ z, const int64_t* __restrict__ target,
                                                        const int32_t* __restrict__ n_valid, float* __restrict__ lse,
                                                        float* __restrict__ row_loss, int32_t* __restrict__ rank,
                                                        int32_t* __restrict__ pred, int64_t B, int C, float eps) {
    __shared__ __attribute__((aligned(16))) float row_s[STAGED ? SCE_LDS_FLOATS : 4];
    __shared__ float red_f[4];
    __shared__ int red_i[4];
    __shared__ float red_m[4];
    const int64_t b = blockIdx.x;
    if (b >= valid_rows(n_valid, B)) return;     // uniform over the workgroup
    const int tid = threadIdx.x;
    const float* zr = z + b * C;
    const int64_t t64 = target[b];
    const bool t_ok = t64 >= 0 && t64 < C;
    const int t = t_ok ? (int)t64 : 0;

    // pass 1: max, lowest arg-max, sum of the logits; stage the row
    float m = -INFINITY, sz = 0.f;
    int mi = INT_MAX;
    if (VEC) {
        const f32x4* zr4 = reinterpret_cast<const f32x4*>(zr);
        for (int q = tid; q < C / 4; q += SCE_THREADS) {
            const f32x4 v = zr4[q];
            if (STAGED) reinterpret_cast<f32x4*>(row_s)[q] = v;
            take_max(v.x, 4 * q, m, mi);
            take_max(v.y, 4 * q + 1, m, mi);
            take_max(v.z, 4 * q + 2, m, mi);
            take_max(v.w, 4 * q + 3, m, mi);
            sz += (v.x + v.y) + (v.z + v.w);
        }
    } else {
        for (int j = tid; j < C; j += SCE_THREADS) {
            const float v = zr[j];
            if (STAGED) row_s[j] = v;
            take_max(v, j, m, mi);
            sz += v;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float om = __shfl_xor(m, o, 64);
        const int oi = __shfl_xor(mi, o, 64);
        if (om > m || (om == m && oi < mi)) { m = om; mi = oi; }
    }
    if (lane_id() == 0) { red_m[tid >> 6] = m; red_i[tid >> 6] = mi; }
    __syncthreads();                             // also publishes the staged row
    m = red_m[0];
    mi = red_i[0];
#pragma unroll
    for (int w = 1; w < 4; ++w) {
        const float om = red_m[w];
        const int oi = red_i[w];
        if (om > m || (om == m && oi < mi)) { m = om; mi = oi; }
    }
    const float* row = STAGED ? row_s : zr;
    const float zt = t_ok ? row[t] : NAN;

    // pass 2: sum exp(z - max) and the target's position in a stable descending sort
    float s = 0.f;
    int cnt = 0;
    if (VEC) {
        const f32x4* r4 = reinterpret_cast<const f32x4*>(row);
        for (int q = tid; q < C / 4; q += SCE_THREADS) {
            const f32x4 v = r4[q];
            const int j = 4 * q;
            s += (expf(v.x - m) + expf(v.y - m)) + (expf(v.z - m) + expf(v.w - m));
            cnt += (v.x > zt || (v.x == zt && j < t)) + (v.y > zt || (v.y == zt && j + 1 < t)) +
                   (v.z > zt || (v.z == zt && j + 2 < t)) + (v.w > zt || (v.w == zt && j + 3 < t));
        }
    } else {
        for (int j = tid; j < C; j += SCE_THREADS) {
            const float v = row[j];
            s += expf(v - m);
            cnt += v > zt || (v == zt && j < t);
        }
    }
    s = block_sum(s, red_f);
    sz = block_sum(sz, red_f);
    cnt = block_sum(cnt, red_i);
    if (tid == 0) {
        const float ls = logf(s);
        const float l = m + ls;                  // NaN for a row with a NaN or +inf logit
        // lse - z_t and lse - mean as (max - .) + log s: the rounding of lse (half an ulp of a number of the logits'
        // size) stays out of a loss that is small when the target holds the maximum
        const float smooth = eps != 0.f ? eps * ((m - sz / (float)C) + ls) : 0.f;
        const bool bad = !t_ok || !(l == l);
        lse[b] = l;
        row_loss[b] = (1.f - eps) * ((m - zt) + ls) + smooth;        // zt is NaN for a bad target
        rank[b] = bad ? C : cnt;
        pred[b] = mi < C ? mi : 0;               // INT_MAX only when no logit compares above -inf
    }
}

__global__ __launch_bounds__(SCE_THREADS) void sce_mean_k(const float* __restrict__ row_loss,
                                                         const int32_t* __restrict__ n_valid, float* __restrict__ loss,
                                                         int64_t B) {
    __shared__ float red_f[4];
    const int64_t nv = valid_rows(n_valid, B);
    float s = 0.f;
    for (int64_t i = threadIdx.x; i < nv; i += SCE_THREADS) s += row_loss[i];
    s = block_sum(s, red_f);
    if (threadIdx.x == 0) loss[0] = s / (float)nv;           // an empty mean is NaN, as torch's
}

template <bool VEC>
__global__ __launch_bounds__(SCE_THREADS) void sce_bwd_k(const float* __restrict__ z, const int64_t* __restrict__ target,
                                                        const int32_t* __restrict__ n_valid, const float* __restrict__ lse,
                                                        const float* __restrict__ g, float* __restrict__ dz, int64_t B,
                                                        int C, float eps) {
    const int64_t b = blockIdx.x;
    const int64_t nv = valid_rows(n_valid, B);
    const int tid = threadIdx.x;
    const float* zr = z + b * C;
    float* dr = dz + b * C;
    const bool live = b < nv;
    const int64_t t64 = live ? target[b] : 0;
    const bool t_ok = t64 >= 0 && t64 < C;
    const int t = t_ok ? (int)t64 : -1;          // -1 matches no column
    const float fill = live ? NAN : 0.f;         // a live row gets here only with a bad target
    if (!live || !t_ok) {
        for (int j = tid; j < C; j += SCE_THREADS) dr[j] = fill;
        return;
    }
    const float scale = g[0] / (float)nv;
    const float l = lse[b];
    const float hit = 1.f - eps, flat = eps / (float)C;
    if (VEC) {
        const f32x4* zr4 = reinterpret_cast<const f32x4*>(zr);
        f32x4* dr4 = reinterpret_cast<f32x4*>(dr);
        for (int q = tid; q < C / 4; q += SCE_THREADS) {
            const f32x4 v = zr4[q];
            const int j = 4 * q;
            f32x4 d;
            d.x = scale * (expf(v.x - l) - (j == t ? hit : 0.f) - flat);
            d.y = scale * (expf(v.y - l) - (j + 1 == t ? hit : 0.f) - flat);
            d.z = scale * (expf(v.z - l) - (j + 2 == t ? hit : 0.f) - flat);
            d.w = scale * (expf(v.w - l) - (j + 3 == t ? hit : 0.f) - flat);
            dr4[q] = d;
        }
    } else {
        for (int j = tid; j < C; j += SCE_THREADS) dr[j] = scale * (expf(zr[j] - l) - (j == t ? hit : 0.f) - flat);
    }
}

// ---- one slice of a padded batch.  The slice holds rows [offset, offset + B) of a batch whose first *n_rows rows are real:
// v = clamp(*n_rows - offset, 0, B) of its rows are live, and every mean is over the batch's *n_rows, not the slice's v
__device__ __forceinline__ int64_t live_rows(const int32_t* n_rows, int64_t offset, int64_t B) {
    const int64_t v = (int64_t)*n_rows - offset;
    return v < 0 ? 0 : (v > B ? B : v);
}

__global__ void bsce_live_k(const int32_t* __restrict__ n_rows, int32_t* __restrict__ live, int64_t offset, int64_t B) {
    if (threadIdx.x == 0) live[0] = (int32_t)live_rows(n_rows, offset, B);
}

__global__ __launch_bounds__(SCE_THREADS) void bsce_sum_k(const float* __restrict__ row_loss,
                                                         const int32_t* __restrict__ rank,
                                                         const int32_t* __restrict__ n_rows, float* __restrict__ loss,
                                                         int64_t* __restrict__ correct, int64_t offset, int64_t B) {
    __shared__ float red_f[4];
    __shared__ int red_i[4];
    const int64_t v = live_rows(n_rows, offset, B);
    float s = 0.f;
    int hit = 0;
    for (int64_t i = threadIdx.x; i < v; i += SCE_THREADS) {
        s += row_loss[i];
        hit += rank[i] == 0;
    }
    s = block_sum(s, red_f);
    hit = block_sum(hit, red_i);
    if (threadIdx.x == 0) {
        loss[0] = v > 0 ? s / (float)*n_rows : 0.f;          // v > 0 implies *n_rows > offset >= 0; an empty slice adds nothing
        correct[0] = hit;
    }
}

template <bool VEC>
__global__ __launch_bounds__(SCE_THREADS) void bsce_bwd_k(const float* __restrict__ z, const int64_t* __restrict__ target,
                                                         const int32_t* __restrict__ n_rows, const float* __restrict__ lse,
                                                         const float* __restrict__ g, float* __restrict__ dz,
                                                         int64_t offset, int64_t B, int C, float eps) {
    const int64_t b = blockIdx.x;
    const int tid = threadIdx.x;
    const float* zr = z + b * C;
    float* dr = dz + b * C;
    const bool live = b < live_rows(n_rows, offset, B);
    const int64_t t64 = live ? target[b] : 0;
    const bool t_ok = t64 >= 0 && t64 < C;
    const int t = t_ok ? (int)t64 : -1;          // -1 matches no column
    const float fill = live ? NAN : 0.f;         // a live row gets here only with a bad target
    if (!live || !t_ok) {
        for (int j = tid; j < C; j += SCE_THREADS) dr[j] = fill;
        return;
    }
    const float scale = g[0] / (float)*n_rows;   // a live row implies *n_rows >= 1
    const float l = lse[b];
    const float hit = 1.f - eps, flat = eps / (float)C;
    if (VEC) {
        const f32x4* zr4 = reinterpret_cast<const f32x4*>(zr);
        f32x4* dr4 = reinterpret_cast<f32x4*>(dr);
        for (int q = tid; q < C / 4; q += SCE_THREADS) {
            const f32x4 v = zr4[q];
            const int j = 4 * q;
            f32x4 d;
            d.x = scale * (expf(v.x - l) - (j == t ? hit : 0.f) - flat);
            d.y = scale * (expf(v.y - l) - (j + 1 == t ? hit : 0.f) - flat);
            d.z = scale * (expf(v.z - l) - (j + 2 == t ? hit : 0.f) - flat);
            d.w = scale * (expf(v.w - l) - (j + 3 == t ? hit : 0.f) - flat);
            dr4[q] = d;
        }
    } else {
        for (int j = tid; j < C; j += SCE_THREADS) dr[j] = scale * (expf(zr[j] - l) - (j == t ? hit : 0.f) - flat);
    }
}

// l a + (1 - l) b and h (p + q) with every operation rounded on its own (the header's __fmul_rn / __fadd_rn are plain
// operators that the compiler may contract to an FMA: contraction is switched off for these bodies instead)
__device__ __forceinline__ float blend_rn(float l, float a, float b) {
#pragma clang fp contract(off)
    const float w = 1.f - l;
    const float x = l * a, y = w * b;
    return x + y;
}
__device__ __forceinline__ float scaled_sum_rn(float h, float p, float q) {
#pragma clang fp contract(off)
    const float s = p + q;
    return h * s;
}

// a x - b y with both products rounded before the subtraction: equal operand pairs give exactly 0, which an FMA would not
__device__ __forceinline__ float product_diff_rn(float a, float x, float b, float y) {
#pragma clang fp contract(off)
    const float p = a * x, q = b * y;
    return p - q;
}

// ---- the same slice with two targets and a weight per row (hwgat_mbsce_*: Mixup / CutMix targets).  sce_fwd_k runs once per
// target; mbsce_sum_k blends the two row losses, keeps the dominant label's rank and then sums as bsce_sum_k does
__global__ __launch_bounds__(SCE_THREADS) void mbsce_sum_k(float* __restrict__ row_loss, const float* __restrict__ row_loss_b,
                                                          int32_t* __restrict__ rank, const int32_t* __restrict__ rank_b,
                                                          const float* __restrict__ lam, const int32_t* __restrict__ n_rows,
                                                          float* __restrict__ loss, int64_t* __restrict__ correct,
                                                          int64_t offset, int64_t B) {
    __shared__ float red_f[4];
    __shared__ int red_i[4];
    const int64_t v = live_rows(n_rows, offset, B);
    float s = 0.f;
    int hit = 0;
    for (int64_t i = threadIdx.x; i < v; i += SCE_THREADS) {
        const float l = lam[i];
        const float r = blend_rn(l, row_loss[i], row_loss_b[i]);
        const int k = l >= 0.5f ? rank[i] : rank_b[i];        // the dominant label's
        row_loss[i] = r;
        rank[i] = k;
        s += r;
        hit += k == 0;
    }
    s = block_sum(s, red_f);
    hit = block_sum(hit, red_i);
    if (threadIdx.x == 0) {
        loss[0] = v > 0 ? s / (float)*n_rows : 0.f;
        correct[0] = hit;
    }
}

template <bool VEC>
__global__ __launch_bounds__(SCE_THREADS) void mbsce_bwd_k(const float* __restrict__ z, const int64_t* __restrict__ target,
                                                          const int64_t* __restrict__ target_b,
                                                          const float* __restrict__ lam, const int32_t* __restrict__ n_rows,
                                                          const float* __restrict__ lse, const float* __restrict__ g,
                                                          float* __restrict__ dz, int64_t offset, int64_t B, int C, float eps) {
    const int64_t b = blockIdx.x;
    const int tid = threadIdx.x;
    const float* zr = z + b * C;
    float* dr = dz + b * C;
    const bool live = b < live_rows(n_rows, offset, B);
    const int64_t t64 = live ? target[b] : 0, u64 = live ? target_b[b] : 0;
    const bool t_ok = t64 >= 0 && t64 < C && u64 >= 0 && u64 < C;
    const int t = t_ok ? (int)t64 : -1, u = t_ok ? (int)u64 : -1;      // -1 matches no column
    const float fill = live ? NAN : 0.f;         // a live row gets here only with a bad target
    if (!live || !t_ok) {
        for (int j = tid; j < C; j += SCE_THREADS) dr[j] = fill;
        return;
    }
    const float scale = g[0] / (float)*n_rows;   // a live row implies *n_rows >= 1
    const float l = lse[b];
    const float hit = 1.f - eps, flat = eps / (float)C;
    const float wa = lam[b], wb = 1.f - wa;
#define MBSCE_HIT(j) (scaled_sum_rn(hit, (j) == t ? wa : 0.f, (j) == u ? wb : 0.f))
    if (VEC) {
        const f32x4* zr4 = reinterpret_cast<const f32x4*>(zr);
        f32x4* dr4 = reinterpret_cast<f32x4*>(dr);
        for (int q = tid; q < C / 4; q += SCE_THREADS) {
            const f32x4 v = zr4[q];
            const int j = 4 * q;
            f32x4 d;
            d.x = scale * (expf(v.x - l) - MBSCE_HIT(j) - flat);
            d.y = scale * (expf(v.y - l) - MBSCE_HIT(j + 1) - flat);
            d.z = scale * (expf(v.z - l) - MBSCE_HIT(j + 2) - flat);
            d.w = scale * (expf(v.w - l) - MBSCE_HIT(j + 3) - flat);
            dr4[q] = d;
        }
    } else {
        for (int j = tid; j < C; j += SCE_THREADS) dr[j] = scale * (expf(zr[j] - l) - MBSCE_HIT(j) - flat);
    }
#undef MBSCE_HIT
}

// ---- the same slice distilled from a teacher (hwgat_kd_*).  state: two device floats, alpha and tau, clamped when read
struct kd_state { float alpha, tau; };
static_assert(sizeof(kd_state) == 8, "the state is two floats");
constexpr int KD_LDS_FLOATS = 4096;            // per row: student and teacher rows of up to 16 KB each are staged in LDS

__device__ __forceinline__ float kd_alpha(const kd_state* st) { return fminf(fmaxf(st->alpha, 0.f), 1.f); }    // a NaN: 0
__device__ __forceinline__ float kd_tau(const kd_state* st) {
    return fminf(fmaxf(st->tau, (float)HWGAT_KD_TAU_MIN), (float)HWGAT_KD_TAU_MAX);                             // a NaN: the minimum
}

__global__ void kd_set_k(kd_state* st, float alpha, float tau) {
    if (threadIdx.x != 0) return;
    st->alpha = alpha;
    st->tau = tau;
}

// one column of a row's KL sums.  a = z/tau - max z/tau and b = u/tau - max u/tau are the exponents of the two softmax
// numerators; d = (u - z)/tau - c with c the difference of the two maxima is delta, shifted so that qn * e^d = e^b <= 1
struct kd_sums { double ss, st, sp, sq; };
__device__ __forceinline__ void kd_term(float z, float u, float tau, float ms, float mt, float c, kd_sums& k) {
    const float qn = expf(z / tau - ms), pn = expf(u / tau - mt);
    k.ss += (double)qn;
    k.st += (double)pn;
    if (u == -INFINITY) {                        // p_j = 0: no term in the KL, and q_j e^delta_j = 0
        k.sq -= (double)qn;
    } else {
        const float d = (u - z) / tau - c;
        k.sp += (double)(pn * d);
        k.sq += (double)(qn * expm1f(d));
    }
}

// row_kd = tau^2 KL(softmax(u/tau) || softmax(z/tau)) = tau^2 (sum_j p_j d_j - log1p(sum_j q_j expm1(d_j))), the four sums
// in double; a row whose u equals z bit for bit has every d_j = 0 and so exactly 0.  alpha == 0: the teacher is not read
template <bool STAGED, bool VEC>
__global__ __launch_bounds__(SCE_THREADS) void kd_row_k(const float* __restrict__ z, const float* __restrict__ u,
                                                       const int32_t* __restrict__ live, const kd_state* __restrict__ state,
                                                       float* __restrict__ lse_s, float* __restrict__ lse_t,
                                                       float* __restrict__ row_kd, int32_t* __restrict__ t_pred, int64_t B,
                                                       int C) {
    __shared__ __attribute__((aligned(16))) float zs[STAGED ? KD_LDS_FLOATS : 4];
    __shared__ __attribute__((aligned(16))) float us[STAGED ? KD_LDS_FLOATS : 4];
    __shared__ double red_d[4];
    __shared__ int red_i[4];
    __shared__ float red_m[4], red_n[4];
    const int64_t b = blockIdx.x;
    if (b >= valid_rows(live, B)) return;        // uniform over the workgroup
    const int tid = threadIdx.x;
    if (kd_alpha(state) == 0.f) {                // the hard loss alone: no soft term, no teacher prediction
        if (tid == 0) { lse_s[b] = 0.f; lse_t[b] = 0.f; row_kd[b] = 0.f; t_pred[b] = -1; }
        return;
    }
    const float tau = kd_tau(state);
    const float* zr = z + b * C;
    const float* ur = u + b * C;

    // pass 1: the student's max, the teacher's max and lowest arg-max; stage both rows
    float mz = -INFINITY, mu = -INFINITY;
    int zi = INT_MAX, ui = INT_MAX;
    if (VEC) {
        const f32x4* zr4 = reinterpret_cast<const f32x4*>(zr);
        const f32x4* ur4 = reinterpret_cast<const f32x4*>(ur);
        for (int q = tid; q < C / 4; q += SCE_THREADS) {
            const f32x4 v = zr4[q], w = ur4[q];
            if (STAGED) { reinterpret_cast<f32x4*>(zs)[q] = v; reinterpret_cast<f32x4*>(us)[q] = w; }
            take_max(v.x, 4 * q, mz, zi); take_max(v.y, 4 * q + 1, mz, zi);
            take_max(v.z, 4 * q + 2, mz, zi); take_max(v.w, 4 * q + 3, mz, zi);
            take_max(w.x, 4 * q, mu, ui); take_max(w.y, 4 * q + 1, mu, ui);
            take_max(w.z, 4 * q + 2, mu, ui); take_max(w.w, 4 * q + 3, mu, ui);
        }
    } else {
        for (int j = tid; j < C; j += SCE_THREADS) {
            const float v = zr[j], w = ur[j];
            if (STAGED) { zs[j] = v; us[j] = w; }
            take_max(v, j, mz, zi);
            take_max(w, j, mu, ui);
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        mz = fmaxf(mz, __shfl_xor(mz, o, 64));
        const float om = __shfl_xor(mu, o, 64);
        const int oi = __shfl_xor(ui, o, 64);
        if (om > mu || (om == mu && oi < ui)) { mu = om; ui = oi; }
    }
    if (lane_id() == 0) { red_n[tid >> 6] = mz; red_m[tid >> 6] = mu; red_i[tid >> 6] = ui; }
    __syncthreads();                             // also publishes the staged rows
    mz = fmaxf(fmaxf(red_n[0], red_n[1]), fmaxf(red_n[2], red_n[3]));
    mu = red_m[0];
    ui = red_i[0];
#pragma unroll
    for (int w = 1; w < 4; ++w) {
        const float om = red_m[w];
        const int oi = red_i[w];
        if (om > mu || (om == mu && oi < ui)) { mu = om; ui = oi; }
    }
    const float ms = mz / tau, mt = mu / tau;    // the maxima of z/tau and u/tau: the division is monotone
    const float c = mt - ms;
    const float* zrow = STAGED ? zs : zr;
    const float* urow = STAGED ? us : ur;

    // pass 2: the four sums
    kd_sums k = {0.0, 0.0, 0.0, 0.0};
    if (VEC) {
        const f32x4* z4 = reinterpret_cast<const f32x4*>(zrow);
        const f32x4* u4 = reinterpret_cast<const f32x4*>(urow);
        for (int q = tid; q < C / 4; q += SCE_THREADS) {
            const f32x4 v = z4[q], w = u4[q];
            kd_term(v.x, w.x, tau, ms, mt, c, k);
            kd_term(v.y, w.y, tau, ms, mt, c, k);
            kd_term(v.z, w.z, tau, ms, mt, c, k);
            kd_term(v.w, w.w, tau, ms, mt, c, k);
        }
    } else {
        for (int j = tid; j < C; j += SCE_THREADS) kd_term(zrow[j], urow[j], tau, ms, mt, c, k);
    }
    const double ss = block_sum(k.ss, red_d);
    const double st = block_sum(k.st, red_d);
    const double sp = block_sum(k.sp, red_d);
    const double sq = block_sum(k.sq, red_d);
    if (tid == 0) {
        lse_s[b] = ms + logf((float)ss);         // the same expression on both sides: equal rows give equal bits
        lse_t[b] = mt + logf((float)st);
        const double kl = sp / st - log1p(sq / ss);
        const bool bad = !(mu == mu) || mu == INFINITY || ui >= C;      // (a NaN never enters the max: the sums carry it)
        row_kd[b] = bad ? NAN : (float)((double)tau * (double)tau * kl);
        t_pred[b] = ui < C ? ui : 0;
    }
}

// blends the hard row loss as mbsce_sum_k does (lam NULL: one target, bsce_sum_k's), mixes in the soft one and takes every
// sum of the slice in bsce_sum_k's order.  alpha == 0 keeps the hard loss's bits whatever row_kd holds
__global__ __launch_bounds__(SCE_THREADS) void kd_sum_k(float* __restrict__ row_loss, const float* __restrict__ row_loss_b,
                                                       int32_t* __restrict__ rank, const int32_t* __restrict__ rank_b,
                                                       const int64_t* __restrict__ target,
                                                       const int64_t* __restrict__ target_b, const float* __restrict__ lam,
                                                       const float* __restrict__ row_kd, const int32_t* __restrict__ pred,
                                                       const int32_t* __restrict__ t_pred,
                                                       const int32_t* __restrict__ n_rows, const kd_state* __restrict__ state,
                                                       float* __restrict__ loss, float* __restrict__ kd,
                                                       int64_t* __restrict__ correct, int64_t* __restrict__ agree,
                                                       int64_t* __restrict__ t_correct, int64_t offset, int64_t B) {
    __shared__ float red_f[4];
    __shared__ int red_i[4];
    const int64_t v = live_rows(n_rows, offset, B);
    const float alpha = kd_alpha(state), hard_w = 1.f - alpha;
    float s = 0.f, sk = 0.f;
    int hit = 0, ag = 0, tc = 0;
    for (int64_t i = threadIdx.x; i < v; i += SCE_THREADS) {
        float h = row_loss[i];
        int k = rank[i];
        int64_t dom = target[i];
        if (lam) {
            const float l = lam[i];
            h = blend_rn(l, h, row_loss_b[i]);
            if (!(l >= 0.5f)) { k = rank_b[i]; dom = target_b[i]; }      // the dominant label's
            rank[i] = k;
        }
        const float rk = row_kd[i];
        const float r = alpha == 0.f ? h : hard_w * h + alpha * rk;
        const int tp = t_pred[i];
        row_loss[i] = r;
        s += r;
        sk += rk;
        hit += k == 0;
        ag += pred[i] == tp;
        tc += tp >= 0 && (int64_t)tp == dom;                      // t_pred is -1 where alpha == 0 left the teacher unread
    }
    s = block_sum(s, red_f);
    sk = block_sum(sk, red_f);
    hit = block_sum(hit, red_i);
    ag = block_sum(ag, red_i);
    tc = block_sum(tc, red_i);
    if (threadIdx.x == 0) {
        loss[0] = v > 0 ? s / (float)*n_rows : 0.f;
        kd[0] = v > 0 ? sk / (float)*n_rows : 0.f;
        correct[0] = hit;
        agree[0] = ag;
        t_correct[0] = tc;
    }
}

// mbsce_bwd_k (lam NULL: weights 1 and 0, which give bsce_bwd_k's bits) plus alpha tau (softmax(z/tau) - softmax(u/tau)),
// the two softmaxes from lse_s / lse_t and renormalised by their own row sums;
// alpha == 0 evaluates mbsce_bwd_k's expression itself and does not read the teacher
template <bool VEC>
__global__ __launch_bounds__(SCE_THREADS) void kd_bwd_k(const float* __restrict__ z, const float* __restrict__ u,
                                                       const int64_t* __restrict__ target,
                                                       const int64_t* __restrict__ target_b, const float* __restrict__ lam,
                                                       const int32_t* __restrict__ n_rows, const kd_state* __restrict__ state,
                                                       const float* __restrict__ lse, const float* __restrict__ lse_s,
                                                       const float* __restrict__ lse_t, const float* __restrict__ g,
                                                       float* __restrict__ dz, int64_t offset, int64_t B, int C, float eps) {
    __shared__ double red_d[4];
    const int64_t b = blockIdx.x;
    const int tid = threadIdx.x;
    const float* zr = z + b * C;
    const float* ur = u + b * C;
    float* dr = dz + b * C;
    const bool live = b < live_rows(n_rows, offset, B);
    const int64_t t64 = live ? target[b] : 0, u64 = live ? (lam ? target_b[b] : target[b]) : 0;
    const bool t_ok = t64 >= 0 && t64 < C && u64 >= 0 && u64 < C;
    const int t = t_ok ? (int)t64 : -1, tb = t_ok ? (int)u64 : -1;     // -1 matches no column
    const float fill = live ? NAN : 0.f;         // a live row gets here only with a bad target
    if (!live || !t_ok) {
        for (int j = tid; j < C; j += SCE_THREADS) dr[j] = fill;
        return;
    }
    const float scale = g[0] / (float)*n_rows;   // a live row implies *n_rows >= 1
    const float l = lse[b];
    const float hit = 1.f - eps, flat = eps / (float)C;
    const float wa = lam ? lam[b] : 1.f, wb = 1.f - wa;
    const float alpha = kd_alpha(state);
#define KD_HIT(j) (scaled_sum_rn(hit, (j) == t ? wa : 0.f, (j) == tb ? wb : 0.f))
    if (alpha == 0.f) {
        if (VEC) {
            const f32x4* zr4 = reinterpret_cast<const f32x4*>(zr);
            f32x4* dr4 = reinterpret_cast<f32x4*>(dr);
            for (int q = tid; q < C / 4; q += SCE_THREADS) {
                const f32x4 v = zr4[q];
                const int j = 4 * q;
                f32x4 d;
                d.x = scale * (expf(v.x - l) - KD_HIT(j) - flat);
                d.y = scale * (expf(v.y - l) - KD_HIT(j + 1) - flat);
                d.z = scale * (expf(v.z - l) - KD_HIT(j + 2) - flat);
                d.w = scale * (expf(v.w - l) - KD_HIT(j + 3) - flat);
                dr4[q] = d;
            }
        } else {
            for (int j = tid; j < C; j += SCE_THREADS) dr[j] = scale * (expf(zr[j] - l) - KD_HIT(j) - flat);
        }
        return;
    }
    const float tau = kd_tau(state), ls = lse_s[b], lt = lse_t[b];
    const float hard_w = 1.f - alpha, soft_w = alpha * tau;
    // the two softmaxes differ by order 1 / tau, and lse_s / lse_t are each rounded to half an ulp of a number of order
    // log C: the rows are normalised again by their own sums (1 up to that rounding), taken in double in the fixed order
    double zs = 0.0, zt = 0.0;
    if (VEC) {
        const f32x4* zr4 = reinterpret_cast<const f32x4*>(zr);
        const f32x4* ur4 = reinterpret_cast<const f32x4*>(ur);
        for (int q = tid; q < C / 4; q += SCE_THREADS) {
            const f32x4 v = zr4[q], w = ur4[q];
            zs += ((double)expf(v.x / tau - ls) + (double)expf(v.y / tau - ls)) + ((double)expf(v.z / tau - ls) + (double)expf(v.w / tau - ls));
            zt += ((double)expf(w.x / tau - lt) + (double)expf(w.y / tau - lt)) + ((double)expf(w.z / tau - lt) + (double)expf(w.w / tau - lt));
        }
    } else {
        for (int j = tid; j < C; j += SCE_THREADS) {
            zs += (double)expf(zr[j] / tau - ls);
            zt += (double)expf(ur[j] / tau - lt);
        }
    }
    zs = block_sum(zs, red_d);
    zt = block_sum(zt, red_d);
    const float ns = (float)(1.0 / zs), nt = (float)(1.0 / zt);      // equal rows: equal bits, an exactly zero soft term
#define KD_D(zv, uv, j) (scale * (hard_w * (expf((zv) - l) - KD_HIT(j) - flat) + soft_w * product_diff_rn(expf((zv) / tau - ls), ns, expf((uv) / tau - lt), nt)))
    if (VEC) {
        const f32x4* zr4 = reinterpret_cast<const f32x4*>(zr);
        const f32x4* ur4 = reinterpret_cast<const f32x4*>(ur);
        f32x4* dr4 = reinterpret_cast<f32x4*>(dr);
        for (int q = tid; q < C / 4; q += SCE_THREADS) {
            const f32x4 v = zr4[q], w = ur4[q];
            const int j = 4 * q;
            f32x4 d;
            d.x = KD_D(v.x, w.x, j);
            d.y = KD_D(v.y, w.y, j + 1);
            d.z = KD_D(v.z, w.z, j + 2);
            d.w = KD_D(v.w, w.w, j + 3);
            dr4[q] = d;
        }
    } else {
        for (int j = tid; j < C; j += SCE_THREADS) dr[j] = KD_D(zr[j], ur[j], j);
    }
#undef KD_D
#undef KD_HIT
}

// accumulator block, in 8-byte words (hwgat_hip.h documents the same offsets)
constexpr int ACC_N_SAMPLES = 0, ACC_N_BATCHES = 1, ACC_N_INVALID = 2, ACC_LOSS_SAMPLES = 3, ACC_LOSS_BATCHES = 4,
              ACC_RANK_HIST = 5;

__global__ __launch_bounds__(SCE_THREADS) void eval_acc_k(int64_t* __restrict__ acc, const float* __restrict__ row_loss,
                                                         const int32_t* __restrict__ rank,
                                                         const int32_t* __restrict__ pred,
                                                         const int64_t* __restrict__ target,
                                                         const float* __restrict__ loss,
                                                         const int32_t* __restrict__ n_valid, int64_t B, int C, int k_max,
                                                         int64_t cap) {
    __shared__ double red_d[4];
    __shared__ int red_i[4];
    const int64_t nv = valid_rows(n_valid, B);
    if (nv == 0) return;                         // an empty batch is no batch
    const int tid = threadIdx.x;
    unsigned long long* hist = reinterpret_cast<unsigned long long*>(acc + ACC_RANK_HIST);
    unsigned long long* conf = hist + (k_max + 1);
    int32_t* pred_log = reinterpret_cast<int32_t*>(conf + (int64_t)C * C);
    int32_t* target_log = pred_log + cap;
    const int64_t base = acc[ACC_N_SAMPLES];     // read by every thread before thread 0 rewrites it (barriers below)
    double s = 0.0;
    int invalid = 0;
    for (int64_t r = tid; r < nv; r += SCE_THREADS) {
        s += (double)row_loss[r];
        const int64_t t = target[r];
        const int p = pred[r];
        const bool t_ok = t >= 0 && t < C;
        if (!t_ok) {
            ++invalid;
        } else {
            int k = rank[r];
            k = k < 0 ? 0 : (k > k_max ? k_max : k);
            atomicAdd(hist + k, 1ull);
            if (p >= 0 && p < C) atomicAdd(conf + t * C + p, 1ull);
        }
        if (base + r < cap) {                    // a full log drops further rows; the counters above still see them
            pred_log[base + r] = p;
            target_log[base + r] = t_ok ? (int32_t)t : -1;
        }
    }
    s = block_sum(s, red_d);
    invalid = block_sum(invalid, red_i);
    if (tid == 0) {
        acc[ACC_N_SAMPLES] = base + nv;
        acc[ACC_N_BATCHES] += 1;
        acc[ACC_N_INVALID] += invalid;
        double* f = reinterpret_cast<double*>(acc);
        f[ACC_LOSS_SAMPLES] += s;
        f[ACC_LOSS_BATCHES] += (double)loss[0];
    }
}

inline bool bad_shape(int64_t B, int C) { return B < 1 || B > 0x7fffffff || C < 1 || C > SCE_MAX_C; }
inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// sce_fwd_k on the first *n_valid rows (all B when NULL): staged in LDS when the row fits, 16-byte loads when it can
inline void launch_sce_rows(const float* logits, const int64_t* target, const int32_t* n_valid, float* lse, float* row_loss,
                            int32_t* rank, int32_t* pred, int64_t B, int C, float eps, hipStream_t st) {
    const bool vec = C % 4 == 0 && aligned16(logits);
    const bool staged = C <= SCE_LDS_FLOATS;
#define SCE_FWD(S, V) sce_fwd_k<S, V><<<(unsigned)B, SCE_THREADS, 0, st>>>(logits, target, n_valid, lse, row_loss, rank, pred, B, C, eps)
    if (staged) { if (vec) SCE_FWD(true, true); else SCE_FWD(true, false); }
    else { if (vec) SCE_FWD(false, true); else SCE_FWD(false, false); }
#undef SCE_FWD
}

inline bool bad_offset(int64_t offset) { return offset < 0 || offset > 0x7fffffff; }

inline bool kd_hyper_ok(float alpha, float tau) {                  // a NaN fails every comparison
    return alpha >= 0.f && alpha <= 1.f && tau >= (float)HWGAT_KD_TAU_MIN && tau <= (float)HWGAT_KD_TAU_MAX;
}

}  // namespace

extern "C" int hwgat_sce_fwd(const float* logits, const int64_t* target, const int32_t* n_valid, float* lse, float* row_loss,
                             int32_t* rank, int32_t* pred, float* loss, int64_t B, int C, float eps, void* stream) {
    if (!logits || !target || !lse || !row_loss || !rank || !pred || !loss) return HWGAT_EINVAL;
    if (bad_shape(B, C)) return HWGAT_ESHAPE;
    hipStream_t st = (hipStream_t)stream;
    launch_sce_rows(logits, target, n_valid, lse, row_loss, rank, pred, B, C, eps, st);
    sce_mean_k<<<1, SCE_THREADS, 0, st>>>(row_loss, n_valid, loss, B);
    HWGAT_LAUNCH_CHECK();
}

extern "C" int hwgat_sce_bwd(const float* logits, const int64_t* target, const int32_t* n_valid, const float* lse,
                             const float* g, float* dlogits, int64_t B, int C, float eps, void* stream) {
    if (!logits || !target || !lse || !g || !dlogits) return HWGAT_EINVAL;
    if (bad_shape(B, C)) return HWGAT_ESHAPE;
    hipStream_t st = (hipStream_t)stream;
    if (C % 4 == 0 && aligned16(logits) && aligned16(dlogits))
        sce_bwd_k<true><<<(unsigned)B, SCE_THREADS, 0, st>>>(logits, target, n_valid, lse, g, dlogits, B, C, eps);
    else
        sce_bwd_k<false><<<(unsigned)B, SCE_THREADS, 0, st>>>(logits, target, n_valid, lse, g, dlogits, B, C, eps);
    HWGAT_LAUNCH_CHECK();
}

extern "C" int64_t hwgat_eval_acc_bytes(int C, int k_max, int64_t cap) {
    if (C < 1 || C > SCE_MAX_C || k_max < 0 || cap < 0) return -1;
    return 8 * (ACC_RANK_HIST + ((int64_t)k_max + 1) + (int64_t)C * C + cap);       // the two int32 logs fill `cap` words
}

extern "C" int hwgat_eval_accumulate(void* acc, const float* row_loss, const int32_t* rank, const int32_t* pred,
                                     const int64_t* target, const float* loss, const int32_t* n_valid, int64_t B, int C,
                                     int k_max, int64_t cap, void* stream) {
    if (!acc || !row_loss || !rank || !pred || !target || !loss || k_max < 0 || cap < 0) return HWGAT_EINVAL;
    if (bad_shape(B, C)) return HWGAT_ESHAPE;
    eval_acc_k<<<1, SCE_THREADS, 0, (hipStream_t)stream>>>(static_cast<int64_t*>(acc), row_loss, rank, pred, target, loss,
                                                          n_valid, B, C, k_max, cap);
    HWGAT_LAUNCH_CHECK();
}

extern "C" int hwgat_bsce_fwd(const float* logits, const int64_t* target, const int32_t* n_rows, int64_t offset, float* lse,
                              float* row_loss, int32_t* rank, int32_t* pred, float* loss, int64_t* correct, int32_t* live,
                              int64_t B, int C, float eps, void* stream) {
    if (!logits || !target || !n_rows || !lse || !row_loss || !rank || !pred || !loss || !correct || !live || bad_offset(offset))
        return HWGAT_EINVAL;
    if (bad_shape(B, C)) return HWGAT_ESHAPE;
    hipStream_t st = (hipStream_t)stream;
    bsce_live_k<<<1, 64, 0, st>>>(n_rows, live, offset, B);
    launch_sce_rows(logits, target, live, lse, row_loss, rank, pred, B, C, eps, st);
    bsce_sum_k<<<1, SCE_THREADS, 0, st>>>(row_loss, rank, n_rows, loss, correct, offset, B);
    HWGAT_LAUNCH_CHECK();
}

extern "C" int hwgat_bsce_bwd(const float* logits, const int64_t* target, const int32_t* n_rows, int64_t offset,
                              const float* lse, const float* g, float* dlogits, int64_t B, int C, float eps, void* stream) {
    if (!logits || !target || !n_rows || !lse || !g || !dlogits || bad_offset(offset)) return HWGAT_EINVAL;
    if (bad_shape(B, C)) return HWGAT_ESHAPE;
    hipStream_t st = (hipStream_t)stream;
    if (C % 4 == 0 && aligned16(logits) && aligned16(dlogits))
        bsce_bwd_k<true><<<(unsigned)B, SCE_THREADS, 0, st>>>(logits, target, n_rows, lse, g, dlogits, offset, B, C, eps);
    else
        bsce_bwd_k<false><<<(unsigned)B, SCE_THREADS, 0, st>>>(logits, target, n_rows, lse, g, dlogits, offset, B, C, eps);
    HWGAT_LAUNCH_CHECK();
}

extern "C" int hwgat_mbsce_fwd(const float* logits, const int64_t* target, const int64_t* target_b, const float* lam,
                               const int32_t* n_rows, int64_t offset, float* lse, float* row_loss, int32_t* rank,
                               int32_t* pred, float* loss, int64_t* correct, int32_t* live, float* row_loss_b,
                               int32_t* rank_b, int64_t B, int C, float eps, void* stream) {
    if (!logits || !target || !target_b || !lam || !n_rows || !lse || !row_loss || !rank || !pred || !loss || !correct ||
        !live || !row_loss_b || !rank_b || bad_offset(offset))
        return HWGAT_EINVAL;
    if (bad_shape(B, C)) return HWGAT_ESHAPE;
    hipStream_t st = (hipStream_t)stream;
    bsce_live_k<<<1, 64, 0, st>>>(n_rows, live, offset, B);
    launch_sce_rows(logits, target_b, live, lse, row_loss_b, rank_b, pred, B, C, eps, st);
    launch_sce_rows(logits, target, live, lse, row_loss, rank, pred, B, C, eps, st);      // lse and pred: the same bits again
    mbsce_sum_k<<<1, SCE_THREADS, 0, st>>>(row_loss, row_loss_b, rank, rank_b, lam, n_rows, loss, correct, offset, B);
    HWGAT_LAUNCH_CHECK();
}

extern "C" int hwgat_mbsce_bwd(const float* logits, const int64_t* target, const int64_t* target_b, const float* lam,
                               const int32_t* n_rows, int64_t offset, const float* lse, const float* g, float* dlogits,
                               int64_t B, int C, float eps, void* stream) {
    if (!logits || !target || !target_b || !lam || !n_rows || !lse || !g || !dlogits || bad_offset(offset)) return HWGAT_EINVAL;
    if (bad_shape(B, C)) return HWGAT_ESHAPE;
    hipStream_t st = (hipStream_t)stream;
    if (C % 4 == 0 && aligned16(logits) && aligned16(dlogits))
        mbsce_bwd_k<true><<<(unsigned)B, SCE_THREADS, 0, st>>>(logits, target, target_b, lam, n_rows, lse, g, dlogits, offset, B, C, eps);
    else
        mbsce_bwd_k<false><<<(unsigned)B, SCE_THREADS, 0, st>>>(logits, target, target_b, lam, n_rows, lse, g, dlogits, offset, B, C, eps);
    HWGAT_LAUNCH_CHECK();
}

extern "C" int64_t hwgat_kd_state_bytes(void) { return (int64_t)sizeof(kd_state); }

extern "C" int hwgat_kd_set(void* state, float alpha, float tau, void* stream) {
    if (!state || (reinterpret_cast<uintptr_t>(state) & 7) != 0) return HWGAT_EINVAL;
    if (!kd_hyper_ok(alpha, tau)) return HWGAT_ESHAPE;
    kd_set_k<<<1, 64, 0, (hipStream_t)stream>>>(static_cast<kd_state*>(state), alpha, tau);
    HWGAT_LAUNCH_CHECK();
}

extern "C" int hwgat_kd_fwd(const float* logits, const float* teacher, const int64_t* target, const int64_t* target_b,
                            const float* lam, const int32_t* n_rows, int64_t offset, const void* state, float* lse,
                            float* row_loss, int32_t* rank, int32_t* pred, float* loss, int64_t* correct, int32_t* live,
                            float* row_loss_b, int32_t* rank_b, float* lse_s, float* lse_t, float* row_kd, int32_t* t_pred,
                            float* kd, int64_t* agree, int64_t* t_correct, int64_t B, int C, float eps, void* stream) {
    if (!logits || !teacher || !target || !n_rows || !state || !lse || !row_loss || !rank || !pred || !loss || !correct ||
        !live || !lse_s || !lse_t || !row_kd || !t_pred || !kd || !agree || !t_correct || bad_offset(offset))
        return HWGAT_EINVAL;
    if ((target_b == nullptr) != (lam == nullptr)) return HWGAT_EINVAL;              // both, or neither: no mixer
    if (lam && (!row_loss_b || !rank_b)) return HWGAT_EINVAL;
    if ((reinterpret_cast<uintptr_t>(state) & 7) != 0) return HWGAT_EINVAL;
    if (bad_shape(B, C)) return HWGAT_ESHAPE;
    hipStream_t st = (hipStream_t)stream;
    const kd_state* ks = static_cast<const kd_state*>(state);
    bsce_live_k<<<1, 64, 0, st>>>(n_rows, live, offset, B);
    if (lam) launch_sce_rows(logits, target_b, live, lse, row_loss_b, rank_b, pred, B, C, eps, st);
    launch_sce_rows(logits, target, live, lse, row_loss, rank, pred, B, C, eps, st);
    const bool vec = C % 4 == 0 && aligned16(logits) && aligned16(teacher);
    const bool staged = C <= KD_LDS_FLOATS;
#define KD_ROW(S, V) kd_row_k<S, V><<<(unsigned)B, SCE_THREADS, 0, st>>>(logits, teacher, live, ks, lse_s, lse_t, row_kd, t_pred, B, C)
    if (staged) { if (vec) KD_ROW(true, true); else KD_ROW(true, false); }
    else { if (vec) KD_ROW(false, true); else KD_ROW(false, false); }
#undef KD_ROW
    kd_sum_k<<<1, SCE_THREADS, 0, st>>>(row_loss, row_loss_b, rank, rank_b, target, target_b, lam, row_kd, pred, t_pred, n_rows,
                                        ks, loss, kd, correct, agree, t_correct, offset, B);
    HWGAT_LAUNCH_CHECK();
}

extern "C" int hwgat_kd_bwd(const float* logits, const float* teacher, const int64_t* target, const int64_t* target_b,
                            const float* lam, const int32_t* n_rows, int64_t offset, const void* state, const float* lse,
                            const float* lse_s, const float* lse_t, const float* g, float* dlogits, int64_t B, int C,
                            float eps, void* stream) {
    if (!logits || !teacher || !target || !n_rows || !state || !lse || !lse_s || !lse_t || !g || !dlogits || bad_offset(offset))
        return HWGAT_EINVAL;
    if ((target_b == nullptr) != (lam == nullptr)) return HWGAT_EINVAL;
    if ((reinterpret_cast<uintptr_t>(state) & 7) != 0) return HWGAT_EINVAL;
    if (bad_shape(B, C)) return HWGAT_ESHAPE;
    hipStream_t st = (hipStream_t)stream;
    const kd_state* ks = static_cast<const kd_state*>(state);
    if (C % 4 == 0 && aligned16(logits) && aligned16(teacher) && aligned16(dlogits))
        kd_bwd_k<true><<<(unsigned)B, SCE_THREADS, 0, st>>>(logits, teacher, target, target_b, lam, n_rows, ks, lse, lse_s, lse_t, g, dlogits, offset, B, C, eps);
    else
        kd_bwd_k<false><<<(unsigned)B, SCE_THREADS, 0, st>>>(logits, teacher, target, target_b, lam, n_rows, ks, lse, lse_s, lse_t, g, dlogits, offset, B, C, eps);
    HWGAT_LAUNCH_CHECK();
}
