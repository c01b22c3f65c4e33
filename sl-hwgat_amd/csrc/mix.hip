// Mixup and temporal CutMix of the pairs of a batch for gfx950 (train.BatchMixer).  The regularisers that mix two clips of
// a batch used to need torch ops on the host side of the captured train step; here they are two launches in front of the
// forward, with every changing value in device words (state, formulas and tags: include/hwgat_hip.h, "Mixup and temporal
// CutMix"), so that draw -> apply are two nodes of the step's HIP graph:
//
//   mix_draw_k   ONE workgroup, a thread per pair: the step's key from (seed, step), a perfect matching of the live rows
//                through the loader's keyed permutation, per pair the apply / mode decisions, lambda0 ~ Beta(alpha, alpha)
//                by Joehnk's method in fp64, the CutMix segment; the per-row records and the pair list; then step += 1.
//   mix_apply_k  a workgroup per (slice of the row, pair): reads both rows of a mixed pair and writes both, in place.
//
// These are latency kernels (a batch is a few MB; an unmixed pair moves nothing).  No atomics and no cross-workgroup
// communication: every word has one writer per launch and every element of x one reader.  Every index formed from a
// device word is reduced to its range before use.  All stores are plain vector stores.
#include <math.h>

#include "common.h"
#include "fused_ops.h"
#include "keyed_perm.h"

namespace {

static_assert(sizeof(hwgat_mix_state) == 40, "the state is 5 words");

constexpr int MIX_THREADS = 256;
constexpr int MIX_MAX_FRAMES = 1 << 20;
constexpr int MIX_BETA_TRIES = 64;
constexpr int APPLY_CHUNK = 4096, APPLY_MAX_SLICES = 64;       // floats of a row one workgroup takes per pass

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }
__device__ __forceinline__ double clamp_alpha(double a) { return fmin(fmax(a, HWGAT_MIX_ALPHA_MIN), 1.0); }   // a NaN: the minimum
__device__ __forceinline__ int live_rows(const int32_t* n_rows, int B) { return n_rows ? clampi(*n_rows, 0, B) : B; }

__global__ void mix_set_k(hwgat_mix_state* st, double prob, double share, double a_mix, double a_cut, int set_counter,
                          uint32_t seed, uint32_t step) {
    if (threadIdx.x != 0) return;
    st->prob = prob;
    st->cutmix_share = share;
    st->mixup_alpha = a_mix;
    st->cutmix_alpha = a_cut;
    if (set_counter) {
        st->seed = seed;
        st->step = step;
    }
}

// (1 - lambda0) T + 0.5 with the difference, the product and the sum rounded on their own (no FMA: see mix_one)
__device__ __forceinline__ double cut_frames(double l0, int T) {
#pragma clang fp contract(off)
    const double share = 1.0 - l0;
    const double frames = share * (double)T;
    return frames + 0.5;
}

__device__ __forceinline__ void write_single(int r, const int64_t* __restrict__ y, int32_t* __restrict__ partner,
                                             float* __restrict__ lam, int32_t* __restrict__ seg, int32_t* __restrict__ mode,
                                             int64_t* __restrict__ y_b) {
    partner[r] = r;
    lam[r] = 1.0f;
    seg[2 * r] = 0;
    seg[2 * r + 1] = 0;
    mode[r] = HWGAT_MIX_NONE;
    y_b[r] = y[r];
}

__global__ __launch_bounds__(MIX_THREADS) void mix_draw_k(hwgat_mix_state* st, const int64_t* __restrict__ y,
                                                         const int32_t* __restrict__ n_rows, int32_t* __restrict__ pairs,
                                                         int32_t* __restrict__ partner, float* __restrict__ lam,
                                                         int32_t* __restrict__ seg, int32_t* __restrict__ mode,
                                                         int64_t* __restrict__ y_b, int B, int T) {
    const int t = threadIdx.x;
    const uint32_t seed = st->seed, step = st->step;
    const double prob = st->prob, share = st->cutmix_share;
    const double a_mix = clamp_alpha(st->mixup_alpha), a_cut = clamp_alpha(st->cutmix_alpha);
    const int n = live_rows(n_rows, B), np = n >> 1;
    __syncthreads();                                          // every thread has the words before thread 0 moves the step
    const uint32_t k_step = mix32(seed, ((uint64_t)HWGAT_MIX_TAG << 32) | (uint64_t)step);
    const uint32_t k_sigma = mix32(k_step, 0ull);

    // the rows without a partner: padding, and the odd one out
    for (int r = n + t; r < B; r += MIX_THREADS) write_single(r, y, partner, lam, seg, mode, y_b);
    if (t == 0 && (n & 1)) write_single(clampi((int)perm(k_sigma, (uint32_t)n, (uint32_t)(n - 1)), 0, n - 1), y, partner, lam, seg, mode, y_b);
    for (int p = np + t; p < max(B >> 1, 1); p += MIX_THREADS) pairs[2 * p] = pairs[2 * p + 1] = -1;

    for (int p = t; p < np; p += MIX_THREADS) {
        const int a = clampi((int)perm(k_sigma, (uint32_t)n, (uint32_t)(2 * p)), 0, n - 1);
        const int b = clampi((int)perm(k_sigma, (uint32_t)n, (uint32_t)(2 * p + 1)), 0, n - 1);
        const uint32_t kp = mix32(k_step, 1ull + (uint64_t)p);
        pairs[2 * p] = a;
        pairs[2 * p + 1] = b;
        if (!(uniform01(kp, HWGAT_MIX_TAG_APPLY, 0u) < prob)) {
            write_single(a, y, partner, lam, seg, mode, y_b);
            write_single(b, y, partner, lam, seg, mode, y_b);
            continue;
        }
        const bool cut = uniform01(kp, HWGAT_MIX_TAG_MODE, 0u) < share;
        const double inv = __ddiv_rn(1.0, cut ? a_cut : a_mix);
        double l0 = 0.5;
        for (int k = 0; k < MIX_BETA_TRIES; ++k) {            // Joehnk: accepted with probability >= 1/2 per try
            const double X = pow(uniform01(kp, HWGAT_MIX_TAG_BETA, 2u * k), inv);
            const double Y = pow(uniform01(kp, HWGAT_MIX_TAG_BETA, 2u * k + 1u), inv);
            const double S = __dadd_rn(X, Y);
            if (S > 0.0 && S <= 1.0) {
                l0 = __ddiv_rn(X, S);
                break;
            }
        }
        float l = (float)l0;
        int t0 = 0, L = 0;
        if (cut) {
            L = clampi((int)floor(cut_frames(l0, T)), 0, T);
            t0 = clampi((int)floor(__dmul_rn(uniform01(kp, HWGAT_MIX_TAG_START, 0u), (double)(T - L + 1))), 0, T - L);
            l = (float)__ddiv_rn((double)(T - L), (double)T);
        }
        const int md = cut ? HWGAT_MIX_CUTMIX : HWGAT_MIX_MIXUP;
        const int64_t ya = y[a], yb = y[b];
        partner[a] = b;
        partner[b] = a;
        lam[a] = lam[b] = l;
        seg[2 * a] = seg[2 * b] = t0;
        seg[2 * a + 1] = seg[2 * b + 1] = L;
        mode[a] = mode[b] = md;
        y_b[a] = yb;
        y_b[b] = ya;
    }
    if (t == 0) st->step = step + 1u;
}

// the new value of an element whose own row holds `own` and whose partner row holds `other`: Mixup blends, CutMix takes the
// partner's.  Each product and the sum is rounded on its own: the header's __fmul_rn / __fadd_rn are plain operators that
// the compiler may contract to an FMA, so contraction is switched off for this body instead
__device__ __forceinline__ float mix_one(float own, float other, float l, float w, bool mixup) {
#pragma clang fp contract(off)
    const float keep = l * own, take = w * other;
    return mixup ? keep + take : other;
}
__device__ __forceinline__ f32x4 mix_four(f32x4 own, f32x4 other, float l, float w, bool mixup) {
    f32x4 r;
    r.x = mix_one(own.x, other.x, l, w, mixup);
    r.y = mix_one(own.y, other.y, l, w, mixup);
    r.z = mix_one(own.z, other.z, l, w, mixup);
    r.w = mix_one(own.w, other.w, l, w, mixup);
    return r;
}

__global__ __launch_bounds__(MIX_THREADS) void mix_apply_k(float* x, const int32_t* __restrict__ pairs,
                                                          const float* __restrict__ lam, const int32_t* __restrict__ seg,
                                                          const int32_t* __restrict__ mode,
                                                          const int32_t* __restrict__ n_rows, int B, int T, int64_t R) {
    const int n = live_rows(n_rows, B), p = blockIdx.y;
    if (p >= (n >> 1)) return;                                // uniform over the workgroup, as every return below
    const int a = pairs[2 * p], b = pairs[2 * p + 1];
    if (a < 0 || a >= n || b < 0 || b >= n || a == b) return;
    const int md = mode[a];
    if (md != HWGAT_MIX_MIXUP && md != HWGAT_MIX_CUTMIX) return;
    const int64_t TR = (int64_t)T * R;
    int64_t s0 = 0, len = TR;
    if (md == HWGAT_MIX_CUTMIX) {
        const int t0 = clampi(seg[2 * a], 0, T), L = clampi(seg[2 * a + 1], 0, T - t0);
        s0 = (int64_t)t0 * R;
        len = (int64_t)L * R;
    }
    float* pa = x + (int64_t)a * TR + s0;
    float* pb = x + (int64_t)b * TR + s0;
    const bool mixup = md == HWGAT_MIX_MIXUP;
    const float l = lam[a], w = 1.0f - l;
    const int64_t first = (int64_t)blockIdx.x * MIX_THREADS + threadIdx.x, stride = (int64_t)gridDim.x * MIX_THREADS;
    if ((((uintptr_t)pa ^ (uintptr_t)pb) & 15) == 0) {         // the two segments share their alignment: 16-byte body
        const int64_t head = min(len, (int64_t)(((16 - ((uintptr_t)pa & 15)) & 15) >> 2));
        const int64_t nv = (len - head) >> 2;
        for (int64_t e = first; e < head; e += stride) {
            const float va = pa[e], vb = pb[e];
            pa[e] = mix_one(va, vb, l, w, mixup);
            pb[e] = mix_one(vb, va, l, w, mixup);
        }
        f32x4* qa = reinterpret_cast<f32x4*>(pa + head);
        f32x4* qb = reinterpret_cast<f32x4*>(pb + head);
        for (int64_t e = first; e < nv; e += stride) {
            const f32x4 va = qa[e], vb = qb[e];
            qa[e] = mix_four(va, vb, l, w, mixup);
            qb[e] = mix_four(vb, va, l, w, mixup);
        }
        for (int64_t e = head + 4 * nv + first; e < len; e += stride) {
            const float va = pa[e], vb = pb[e];
            pa[e] = mix_one(va, vb, l, w, mixup);
            pb[e] = mix_one(vb, va, l, w, mixup);
        }
    } else {
        for (int64_t e = first; e < len; e += stride) {
            const float va = pa[e], vb = pb[e];
            pa[e] = mix_one(va, vb, l, w, mixup);
            pb[e] = mix_one(vb, va, l, w, mixup);
        }
    }
}

bool aligned(const void* p, uintptr_t a) { return (((uintptr_t)p) & (a - 1)) == 0; }
bool unit(double v) { return v >= 0.0 && v <= 1.0; }                                  // a NaN fails
bool alpha_ok(double v) { return v >= HWGAT_MIX_ALPHA_MIN && v <= 1.0; }
bool sizes_ok(int B, int T) { return B <= HWGAT_MIX_MAX_BATCH && T <= MIX_MAX_FRAMES; }

}  // namespace

extern "C" int64_t hwgat_mix_state_bytes(void) { return (int64_t)sizeof(hwgat_mix_state); }

extern "C" int hwgat_mix_set(void* state, double prob, double cutmix_share, double mixup_alpha, double cutmix_alpha,
                             int set_counter, uint32_t seed, uint32_t step, void* stream) {
    if (!state || !aligned(state, 8)) return HWGAT_EINVAL;
    if (!unit(prob) || !unit(cutmix_share) || !alpha_ok(mixup_alpha) || !alpha_ok(cutmix_alpha)) return HWGAT_ESHAPE;
    mix_set_k<<<1, 64, 0, (hipStream_t)stream>>>(static_cast<hwgat_mix_state*>(state), prob, cutmix_share, mixup_alpha,
                                                 cutmix_alpha, set_counter, seed, step);
    HWGAT_LAUNCH_CHECK();
}

extern "C" int hwgat_mix_draw(void* state, const int64_t* y, const int32_t* n_rows, int32_t* pairs, int32_t* partner,
                              float* lam, int32_t* seg, int32_t* mode, int64_t* y_b, int B, int T, void* stream) {
    if (!state || !aligned(state, 8) || !y || !aligned(y, 8) || !pairs || !partner || !lam || !seg || !mode || !y_b ||
        !aligned(y_b, 8) || B <= 0 || T <= 0)
        return HWGAT_EINVAL;
    if (!sizes_ok(B, T)) return HWGAT_ESHAPE;
    mix_draw_k<<<1, MIX_THREADS, 0, (hipStream_t)stream>>>(static_cast<hwgat_mix_state*>(state), y, n_rows, pairs, partner,
                                                           lam, seg, mode, y_b, B, T);
    HWGAT_LAUNCH_CHECK();
}

extern "C" int hwgat_mix_apply(float* x, const int32_t* pairs, const float* lam, const int32_t* seg, const int32_t* mode,
                               const int32_t* n_rows, int B, int T, int64_t R, void* stream) {
    if (!x || !aligned(x, 4) || !pairs || !lam || !seg || !mode || B <= 0 || T <= 0 || R <= 0) return HWGAT_EINVAL;
    if (!sizes_ok(B, T) || R > (int64_t)INT32_MAX || (int64_t)T * R >= (int64_t)INT32_MAX) return HWGAT_ESHAPE;
    if (B < 2) return 0;                                      // one row has no pair: nothing to launch
    const int64_t want = ((int64_t)T * R + APPLY_CHUNK - 1) / APPLY_CHUNK;
    const unsigned slices = (unsigned)(want < APPLY_MAX_SLICES ? want : APPLY_MAX_SLICES);
    mix_apply_k<<<dim3(slices, (unsigned)(B >> 1)), MIX_THREADS, 0, (hipStream_t)stream>>>(x, pairs, lam, seg, mode, n_rows, B,
                                                                                          T, R);
    HWGAT_LAUNCH_CHECK();
}
