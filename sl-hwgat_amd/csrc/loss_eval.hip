// Smoothed cross-entropy on the classifier's logits and the device-side evaluation accumulators (reference:
// hwgat/losses/SmoothCrossEntropy.py, hwgat/utils.py:118-161 evaluate / predictions_plus_true, :324-350 gen_cm_w).
//
// The four criteria are one: a row rule (loss_rows: a whole batch, or one slice of a padded batch), an optional partner
// target with a weight per row, and an optional teacher.  The eight entry points check their arguments, fill one LossArgs
// and go through loss_fwd / loss_bwd, which hold every launch of the family.
//
//   hwgat_sce_fwd          sce_fwd_k: one workgroup per row -- max / arg-max / sum z, then sum exp / rank count; the row is
//                          staged in LDS when it fits (C <= SCE_LDS_FLOATS), else read twice; 16-byte loads when
//                          C % 4 == 0.  loss_sum_k (one workgroup) then takes the mean of the row losses in a fixed order.
//   hwgat_sce_bwd          loss_bwd_k: one pass over the logits with the stored lse.
//   hwgat_eval_accumulate  eval_acc_k: one workgroup folds a batch into the accumulator block (layout: hwgat_hip.h).
//   hwgat_bsce_fwd         the loss of one SLICE of a padded batch (train.BatchSlicedCrossEntropyLoss): bsce_live_k turns
//                          the batch's row count and the slice's offset into the slice's live-row count, sce_fwd_k runs
//                          on those rows, loss_sum_k adds their losses in the same fixed order, divides by the BATCH's
//                          row count and counts the live rows whose target ranks first.
//   hwgat_bsce_bwd         loss_bwd_k with the batch's row count as the divisor; exact zeros for the other rows.
//   hwgat_mbsce_fwd / _bwd the same slice with two targets and a weight per row (train.MixedCrossEntropyLoss): sce_fwd_k
//                          once per target, loss_sum_k blends the row losses before it sums; loss_bwd_k's one-hot becomes
//                          lam [j == t] + (1 - lam) [j == t_b].
//   hwgat_kd_fwd / _bwd    the same slice with a teacher's logits beside the labels (train.DistilledCrossEntropyLoss):
//                          sce_fwd_k once per target as above, kd_row_k (one workgroup per row, both rows staged in LDS
//                          when C <= KD_LDS_FLOATS) the tempered KL of the row, loss_sum_k the blend and every sum;
//                          loss_bwd_k<.., CE_KD, ..> adds the soft term.  alpha and tau are device words (hwgat_kd_set).
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

// the rows that take part, and what their sum is divided by.
//   batch form   the first *count of the B rows, clamped to [0, B]; all B when the pointer is NULL.  The mean is over them:
//                an empty mean is NaN, as torch's
//   slice form   the B rows are rows [offset, offset + B) of a padded batch whose first *count rows are real:
//                clamp(*count - offset, 0, B) of them are live, and every mean is over the batch's *count, not over the
//                slice's live rows; an empty slice adds nothing, exactly 0
struct loss_rows {
    const int32_t* count;
    int64_t offset;                              // 0 in batch form
    bool slice;
    __device__ __forceinline__ int64_t live(int64_t B) const {
        if (!slice && !count) return B;
        const int64_t n = (int64_t)*count - offset;
        return n < 0 ? 0 : (n > B ? B : n);
    }
    __device__ __forceinline__ float divisor(int64_t v) const { return slice ? (float)*count : (float)v; }
    // v > 0 implies *count > offset >= 0 in slice form
    __device__ __forceinline__ float mean(float s, int64_t v) const { return slice && v == 0 ? 0.f : s / divisor(v); }
};
__device__ __forceinline__ loss_rows batch_rows(const int32_t* n_valid) { return {n_valid, 0, false}; }

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
    if (b >= batch_rows(n_valid).live(B)) return;        // uniform over the workgroup
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

// a slice's live-row count as a device word: what sce_fwd_k and kd_row_k take for their n_valid
__global__ void bsce_live_k(const int32_t* __restrict__ n_rows, int32_t* __restrict__ live, int64_t offset, int64_t B) {
    if (threadIdx.x == 0) live[0] = (int32_t)loss_rows{n_rows, offset, true}.live(B);
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
    if (b >= batch_rows(live).live(B)) return;   // uniform over the workgroup
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

// what the sum and the backward kernel are compiled for: one target; a partner target with a weight per row; a teacher
// (with or without a partner: lam NULL says which, at run time).  The forms are template arguments, and so is the row
// rule's batch / slice flag, because these kernels run for two or three microseconds: a test of an optional pointer is a
// scalar load and a branch in front of the first row, and the one-target forms are the ones every step runs
enum { CE_PLAIN, CE_PAIR, CE_KD };

// ---- the sums of every forward, one workgroup, every floating-point sum in the same fixed order.
//   CE_PAIR  the row loss becomes lam l(t) + (1 - lam) l(t_b), the rank the dominant label's (t when lam >= 0.5); both are
//            written back
//   CE_KD    the soft term is mixed in and written back as well; alpha == 0 keeps the hard loss's bits whatever row_kd
//            holds; kd / agree / t_correct
//   SLICE    the slice's row rule, and `correct`: the number of live rows whose (dominant) target ranks first
// CE_PLAIN writes nothing back: row_loss and rank already hold these bits
template <int FORM, bool SLICE>
__global__ __launch_bounds__(SCE_THREADS) void loss_sum_k(float* __restrict__ row_loss, const float* __restrict__ row_loss_b,
                                                         int32_t* __restrict__ rank, const int32_t* __restrict__ rank_b,
                                                         const int64_t* __restrict__ target,
                                                         const int64_t* __restrict__ target_b, const float* __restrict__ lam,
                                                         const float* __restrict__ row_kd, const int32_t* __restrict__ pred,
                                                         const int32_t* __restrict__ t_pred, const int32_t* __restrict__ count,
                                                         const kd_state* __restrict__ state, float* __restrict__ loss,
                                                         float* __restrict__ kd, int64_t* __restrict__ correct,
                                                         int64_t* __restrict__ agree, int64_t* __restrict__ t_correct,
                                                         int64_t offset, int64_t B) {
    __shared__ float red_f[4];
    __shared__ int red_i[4];
    constexpr bool soft = FORM == CE_KD;
    const loss_rows rows{count, offset, SLICE};
    const bool pair = FORM == CE_PAIR || (soft && lam);
    const int64_t v = rows.live(B);
    const float alpha = soft ? kd_alpha(state) : 0.f, hard_w = 1.f - alpha;      // these and sk / ag / tc: CE_KD alone
    float s = 0.f, sk = 0.f;
    int hit = 0, ag = 0, tc = 0;
    for (int64_t i = threadIdx.x; i < v; i += SCE_THREADS) {
        float h = row_loss[i];
        int k = SLICE ? rank[i] : 0;
        bool first = true;                       // the dominant label is `target`'s
        if (pair) {
            const float l = lam[i];
            h = blend_rn(l, h, row_loss_b[i]);
            first = l >= 0.5f;
            if (!first) k = rank_b[i];
            rank[i] = k;
        }
        float r = h;
        if (soft) {
            const float rk = row_kd[i];
            const int tp = t_pred[i];
            const int64_t dom = first ? target[i] : target_b[i];
            r = alpha == 0.f ? h : hard_w * h + alpha * rk;
            sk += rk;
            ag += pred[i] == tp;
            tc += tp >= 0 && (int64_t)tp == dom;                      // t_pred is -1 where alpha == 0 left the teacher unread
        }
        if (FORM != CE_PLAIN) row_loss[i] = r;
        s += r;
        if (SLICE) hit += k == 0;
    }
    s = block_sum(s, red_f);
    if (soft) sk = block_sum(sk, red_f);
    if (SLICE) hit = block_sum(hit, red_i);
    if (soft) {
        ag = block_sum(ag, red_i);
        tc = block_sum(tc, red_i);
    }
    if (threadIdx.x == 0) {
        loss[0] = rows.mean(s, v);
        if (SLICE) correct[0] = hit;
        if (soft) {
            kd[0] = rows.mean(sk, v);
            agree[0] = ag;
            t_correct[0] = tc;
        }
    }
}

// ---- the backward of every form, one workgroup per row, one launch: dz_j = g / divisor (exp(z_j - lse) - (1 - eps) hit_j -
// eps / C).  CE_PLAIN: hit_j = [j == t].  The other forms: hit_j = wa [j == t] + wb [j == tb] with both operations rounded
// on their own; without a partner (CE_KD, lam NULL) wa = 1, wb = 0 and tb = t, which give the plain one-hot's bits.
// A dead row gets exact zeros, a live row with a bad target NaN
#define CE_HIT(j) (FORM == CE_PLAIN ? ((j) == t ? hit : 0.f) : scaled_sum_rn(hit, (j) == t ? wa : 0.f, (j) == tb ? wb : 0.f))
template <bool VEC, int FORM>
__device__ __forceinline__ void hard_row(const float* __restrict__ zr, float* __restrict__ dr, int C, float scale, float l,
                                         float hit, float flat, int t, int tb, float wa, float wb) {
    const int tid = threadIdx.x;
    if (VEC) {
        const f32x4* zr4 = reinterpret_cast<const f32x4*>(zr);
        f32x4* dr4 = reinterpret_cast<f32x4*>(dr);
        for (int q = tid; q < C / 4; q += SCE_THREADS) {
            const f32x4 v = zr4[q];
            const int j = 4 * q;
            f32x4 d;
            d.x = scale * (expf(v.x - l) - CE_HIT(j) - flat);
            d.y = scale * (expf(v.y - l) - CE_HIT(j + 1) - flat);
            d.z = scale * (expf(v.z - l) - CE_HIT(j + 2) - flat);
            d.w = scale * (expf(v.w - l) - CE_HIT(j + 3) - flat);
            dr4[q] = d;
        }
    } else {
        for (int j = tid; j < C; j += SCE_THREADS) dr[j] = scale * (expf(zr[j] - l) - CE_HIT(j) - flat);
    }
}

// CE_KD: a teacher's logits u, with state / lse_s / lse_t.  The row gets (1 - alpha) times the hard term plus
// alpha tau (softmax(z/tau) - softmax(u/tau)), the two softmaxes from lse_s / lse_t and renormalised by their own row sums;
// alpha == 0 evaluates the hard expression itself and does not read the teacher.  The soft path's doubles and its LDS
// exist in that form alone
template <bool VEC, int FORM, bool SLICE>
__global__ __launch_bounds__(SCE_THREADS) void loss_bwd_k(const float* __restrict__ z, const float* __restrict__ u,
                                                         const int64_t* __restrict__ target,
                                                         const int64_t* __restrict__ target_b, const float* __restrict__ lam,
                                                         const int32_t* __restrict__ count, const kd_state* __restrict__ state,
                                                         const float* __restrict__ lse, const float* __restrict__ lse_s,
                                                         const float* __restrict__ lse_t, const float* __restrict__ g,
                                                         float* __restrict__ dz, int64_t offset, int64_t B, int C, float eps) {
    constexpr bool KD = FORM == CE_KD;
    const loss_rows rows{count, offset, SLICE};
    const bool pair = FORM == CE_PAIR || (KD && lam);
    const int64_t b = blockIdx.x;
    const int tid = threadIdx.x;
    const float* zr = z + b * C;
    float* dr = dz + b * C;
    const int64_t nv = rows.live(B);
    const bool live = b < nv;
    const int64_t t64 = live ? target[b] : 0, u64 = pair && live ? target_b[b] : t64;
    const bool t_ok = t64 >= 0 && t64 < C && u64 >= 0 && u64 < C;
    const int t = t_ok ? (int)t64 : -1, tb = t_ok ? (int)u64 : -1;     // -1 matches no column
    const float fill = live ? NAN : 0.f;         // a live row gets here only with a bad target
    if (!live || !t_ok) {
        for (int j = tid; j < C; j += SCE_THREADS) dr[j] = fill;
        return;
    }
    const float scale = g[0] / rows.divisor(nv); // a live row implies a divisor of at least 1
    const float l = lse[b];
    const float hit = 1.f - eps, flat = eps / (float)C;
    const float wa = pair ? lam[b] : 1.f, wb = 1.f - wa;
    if constexpr (!KD) {
        hard_row<VEC, FORM>(zr, dr, C, scale, l, hit, flat, t, tb, wa, wb);
    } else {
        __shared__ double red_d[4];
        const float alpha = kd_alpha(state);
        if (alpha == 0.f) {
            hard_row<VEC, FORM>(zr, dr, C, scale, l, hit, flat, t, tb, wa, wb);
            return;
        }
        const float* ur = u + b * C;
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
#define KD_D(zv, uv, j) (scale * (hard_w * (expf((zv) - l) - CE_HIT(j) - flat) + soft_w * product_diff_rn(expf((zv) / tau - ls), ns, expf((uv) / tau - lt), nt)))
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
    }
}
#undef CE_HIT

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
    const int64_t nv = batch_rows(n_valid).live(B);
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
inline bool bad_offset(int64_t offset) { return offset < 0 || offset > 0x7fffffff; }

inline bool kd_hyper_ok(float alpha, float tau) {                  // a NaN fails every comparison
    return alpha >= 0.f && alpha <= 1.f && tau >= (float)HWGAT_KD_TAU_MIN && tau <= (float)HWGAT_KD_TAU_MAX;
}

// one launch record for the eight entry points, in hwgat_kd_fwd's order.  Optional things are NULL pointers and the
// options follow from the record and nothing else: `slice` with count / offset is the row rule (loss_rows), target_b / lam
// the partner (both or neither), teacher the teacher.  The forward writes lse / lse_s / lse_t; the backward reads its
// own const members (bwd_lse, bwd_lse_s, bwd_lse_t) beside g and dlogits
struct LossArgs {
    const float* logits; const float* teacher; const int64_t* target; const int64_t* target_b; const float* lam;
    const int32_t* count; int64_t offset; bool slice; const void* state;
    float* lse; float* row_loss; int32_t* rank; int32_t* pred; float* loss; int64_t* correct; int32_t* live;
    float* row_loss_b; int32_t* rank_b; float* lse_s; float* lse_t; float* row_kd; int32_t* t_pred;
    float* kd; int64_t* agree; int64_t* t_correct;
    const float* bwd_lse; const float* bwd_lse_s; const float* bwd_lse_t; const float* g; float* dlogits;
    int64_t B; int C; float eps;
    bool pair() const { return lam != nullptr; }
    bool kd_form() const { return teacher != nullptr; }
    int form() const { return kd_form() ? CE_KD : pair() ? CE_PAIR : CE_PLAIN; }
    const kd_state* words() const { return static_cast<const kd_state*>(state); }
    // 16-byte loads and stores need rows of whole float4s and every buffer the operation touches on a 16-byte boundary
    bool vec(const void* p, const void* q = nullptr) const { return C % 4 == 0 && aligned16(logits) && aligned16(p) && aligned16(q); }
};

// bsce_live_k for a slice, sce_fwd_k once per target, kd_row_k with a teacher, loss_sum_k: 2 to 5 launches
int loss_fwd(const LossArgs& a, hipStream_t st) {
    const int32_t* n_live = a.count;             // the row count that sce_fwd_k and kd_row_k take: the batch's, or the slice's
    if (a.slice) {
        bsce_live_k<<<1, 64, 0, st>>>(a.count, a.live, a.offset, a.B);
        n_live = a.live;
    }
    // sce_fwd_k on the first *n_live rows (all B when NULL): staged in LDS when the row fits, 16-byte loads when it can
    auto sce_rows = [&](const int64_t* target, float* row_loss, int32_t* rank) {
#define SCE_FWD(S, V) sce_fwd_k<S, V><<<(unsigned)a.B, SCE_THREADS, 0, st>>>(a.logits, target, n_live, a.lse, row_loss, rank, a.pred, a.B, a.C, a.eps)
        if (a.C <= SCE_LDS_FLOATS) { if (a.vec(nullptr)) SCE_FWD(true, true); else SCE_FWD(true, false); }
        else { if (a.vec(nullptr)) SCE_FWD(false, true); else SCE_FWD(false, false); }
#undef SCE_FWD
    };
    if (a.pair()) sce_rows(a.target_b, a.row_loss_b, a.rank_b);
    sce_rows(a.target, a.row_loss, a.rank);      // lse and pred: the same bits again
    if (a.kd_form()) {
#define KD_ROW(S, V) kd_row_k<S, V><<<(unsigned)a.B, SCE_THREADS, 0, st>>>(a.logits, a.teacher, n_live, a.words(), a.lse_s, a.lse_t, a.row_kd, a.t_pred, a.B, a.C)
        if (a.C <= KD_LDS_FLOATS) { if (a.vec(a.teacher)) KD_ROW(true, true); else KD_ROW(true, false); }
        else { if (a.vec(a.teacher)) KD_ROW(false, true); else KD_ROW(false, false); }
#undef KD_ROW
    }
    // a partner or a teacher comes with a slice: the entry points have no other form
#define LOSS_SUM(F, S) loss_sum_k<F, S><<<1, SCE_THREADS, 0, st>>>(a.row_loss, a.row_loss_b, a.rank, a.rank_b, a.target, a.target_b, a.lam, a.row_kd, a.pred, a.t_pred, a.count, a.words(), a.loss, a.kd, a.correct, a.agree, a.t_correct, a.offset, a.B)
    switch (a.form()) {
        case CE_KD: LOSS_SUM(CE_KD, true); break;
        case CE_PAIR: LOSS_SUM(CE_PAIR, true); break;
        default: if (a.slice) LOSS_SUM(CE_PLAIN, true); else LOSS_SUM(CE_PLAIN, false);
    }
#undef LOSS_SUM
    HWGAT_LAUNCH_CHECK();
}

int loss_bwd(const LossArgs& a, hipStream_t st) {
    const bool vec = a.vec(a.dlogits, a.teacher);
#define LOSS_BWD(F, S) do { if (vec) LOSS_BWD_(true, F, S); else LOSS_BWD_(false, F, S); } while (0)
#define LOSS_BWD_(V, F, S) loss_bwd_k<V, F, S><<<(unsigned)a.B, SCE_THREADS, 0, st>>>(a.logits, a.teacher, a.target, a.target_b, a.lam, a.count, a.words(), a.bwd_lse, a.bwd_lse_s, a.bwd_lse_t, a.g, a.dlogits, a.offset, a.B, a.C, a.eps)
    switch (a.form()) {
        case CE_KD: LOSS_BWD(CE_KD, true); break;
        case CE_PAIR: LOSS_BWD(CE_PAIR, true); break;
        default: if (a.slice) LOSS_BWD(CE_PLAIN, true); else LOSS_BWD(CE_PLAIN, false);
    }
#undef LOSS_BWD_
#undef LOSS_BWD
    HWGAT_LAUNCH_CHECK();
}

}  // namespace

// ---- the entry points: each checks what it takes, in its own order (the first failing check names the return code), fills
// the record and leaves the rest to the dispatch above
extern "C" int hwgat_sce_fwd(const float* logits, const int64_t* target, const int32_t* n_valid, float* lse, float* row_loss,
                             int32_t* rank, int32_t* pred, float* loss, int64_t B, int C, float eps, void* stream) {
    if (!logits || !target || !lse || !row_loss || !rank || !pred || !loss) return HWGAT_EINVAL;
    if (bad_shape(B, C)) return HWGAT_ESHAPE;
    return loss_fwd({.logits = logits, .target = target, .count = n_valid, .lse = lse, .row_loss = row_loss, .rank = rank,
                     .pred = pred, .loss = loss, .B = B, .C = C, .eps = eps}, (hipStream_t)stream);
}

extern "C" int hwgat_sce_bwd(const float* logits, const int64_t* target, const int32_t* n_valid, const float* lse,
                             const float* g, float* dlogits, int64_t B, int C, float eps, void* stream) {
    if (!logits || !target || !lse || !g || !dlogits) return HWGAT_EINVAL;
    if (bad_shape(B, C)) return HWGAT_ESHAPE;
    return loss_bwd({.logits = logits, .target = target, .count = n_valid, .bwd_lse = lse, .g = g, .dlogits = dlogits,
                     .B = B, .C = C, .eps = eps}, (hipStream_t)stream);
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
    return loss_fwd({.logits = logits, .target = target, .count = n_rows, .offset = offset, .slice = true, .lse = lse,
                     .row_loss = row_loss, .rank = rank, .pred = pred, .loss = loss, .correct = correct, .live = live, .B = B,
                     .C = C, .eps = eps}, (hipStream_t)stream);
}

extern "C" int hwgat_bsce_bwd(const float* logits, const int64_t* target, const int32_t* n_rows, int64_t offset,
                              const float* lse, const float* g, float* dlogits, int64_t B, int C, float eps, void* stream) {
    if (!logits || !target || !n_rows || !lse || !g || !dlogits || bad_offset(offset)) return HWGAT_EINVAL;
    if (bad_shape(B, C)) return HWGAT_ESHAPE;
    return loss_bwd({.logits = logits, .target = target, .count = n_rows, .offset = offset, .slice = true,
                     .bwd_lse = lse, .g = g, .dlogits = dlogits, .B = B, .C = C, .eps = eps}, (hipStream_t)stream);
}

extern "C" int hwgat_mbsce_fwd(const float* logits, const int64_t* target, const int64_t* target_b, const float* lam,
                               const int32_t* n_rows, int64_t offset, float* lse, float* row_loss, int32_t* rank,
                               int32_t* pred, float* loss, int64_t* correct, int32_t* live, float* row_loss_b,
                               int32_t* rank_b, int64_t B, int C, float eps, void* stream) {
    if (!logits || !target || !target_b || !lam || !n_rows || !lse || !row_loss || !rank || !pred || !loss || !correct ||
        !live || !row_loss_b || !rank_b || bad_offset(offset))
        return HWGAT_EINVAL;
    if (bad_shape(B, C)) return HWGAT_ESHAPE;
    return loss_fwd({.logits = logits, .target = target, .target_b = target_b, .lam = lam, .count = n_rows, .offset = offset,
                     .slice = true, .lse = lse, .row_loss = row_loss, .rank = rank, .pred = pred, .loss = loss,
                     .correct = correct, .live = live, .row_loss_b = row_loss_b, .rank_b = rank_b, .B = B, .C = C, .eps = eps},
                    (hipStream_t)stream);
}

extern "C" int hwgat_mbsce_bwd(const float* logits, const int64_t* target, const int64_t* target_b, const float* lam,
                               const int32_t* n_rows, int64_t offset, const float* lse, const float* g, float* dlogits,
                               int64_t B, int C, float eps, void* stream) {
    if (!logits || !target || !target_b || !lam || !n_rows || !lse || !g || !dlogits || bad_offset(offset)) return HWGAT_EINVAL;
    if (bad_shape(B, C)) return HWGAT_ESHAPE;
    return loss_bwd({.logits = logits, .target = target, .target_b = target_b, .lam = lam, .count = n_rows, .offset = offset,
                     .slice = true, .bwd_lse = lse, .g = g, .dlogits = dlogits, .B = B, .C = C, .eps = eps},
                    (hipStream_t)stream);
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
    return loss_fwd({.logits = logits, .teacher = teacher, .target = target, .target_b = target_b, .lam = lam,
                     .count = n_rows, .offset = offset, .slice = true, .state = state, .lse = lse, .row_loss = row_loss,
                     .rank = rank, .pred = pred, .loss = loss, .correct = correct, .live = live, .row_loss_b = row_loss_b,
                     .rank_b = rank_b, .lse_s = lse_s, .lse_t = lse_t, .row_kd = row_kd, .t_pred = t_pred, .kd = kd,
                     .agree = agree, .t_correct = t_correct, .B = B, .C = C, .eps = eps}, (hipStream_t)stream);
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
    return loss_bwd({.logits = logits, .teacher = teacher, .target = target, .target_b = target_b, .lam = lam,
                     .count = n_rows, .offset = offset, .slice = true, .state = state, .bwd_lse = lse,
                     .bwd_lse_s = lse_s, .bwd_lse_t = lse_t, .g = g, .dlogits = dlogits, .B = B, .C = C, .eps = eps},
                    (hipStream_t)stream);
}
