// Adam / AdamW for every parameter tensor of a model in ONE launch on gfx950, driven by a table in device memory (the
// idiom of hwgat_weight_prep, prep.hip), with every hyper-parameter in device words that the kernels read when they run
// (the idiom of the dropout seed, embed.hip: hwgat_seed_set / hwgat_seed_advance).  A train step captured in a HIP
// graph can therefore hold its optimizer: a new learning rate reaches a replay through hwgat_optim_set, a launch of its own
// outside the graph, and nothing of the step is frozen at capture.
//
// Reference: torch.optim.AdamW / Adam as the reference's loop calls them (hwgat/utils.py:71-82, 93-116), amsgrad and
// maximize off, fp32 parameters, gradients and moments:
//     p *= 1 - lr wd   (AdamW)    |    g += wd p   (Adam)
//     m  = m + (1 - b1) (g - m)
//     v  = b2 v + (1 - b2) g g
//     p -= (lr / (1 - b1^t)) m / (sqrt(v) / sqrt(1 - b2^t) + eps)
// Three kernels.  optim_set_k writes one group's hyper-parameters, fp64, from kernel arguments.  optim_advance_k, one
// thread per table entry, adds 1 to the entry's step count and derives the entry's fp32 scalars from the fp64 block (the
// two pow() and the divisions are done once per tensor, not once per workgroup).  optim_step_k streams the four arrays.
// No float atomics, no reductions: the result is a pure function of its inputs.
//
// With a gradient guard (grad_guard.hip) the advance and step kernels are instantiated a second time, GUARD = true, with
// the guard's state block as one more argument: both return at once when its `skip` word is set, so a step whose
// gradients hold a NaN or an Inf changes neither a step count nor a parameter nor a moment.  The GUARD = false
// instantiations take no such argument and hold no trace of the guard: hwgat_optim_{advance,step} launch those.
#include "common.h"

namespace {

constexpr int THREADS = 256;
constexpr int VEC_PER_THREAD = HWGAT_OPTIM_CHUNK / (THREADS * 4);
static_assert(VEC_PER_THREAD * THREADS * 4 == HWGAT_OPTIM_CHUNK, "a chunk is a whole number of 16-byte vectors per thread");
static_assert(sizeof(hwgat_optim_entry) == 56, "the host packs 56-byte records (sl-hwgat_amd/optim.py)");

// slots of an entry's derived block
constexpr int D_LRWD = 0, D_WD = 1, D_OMB1 = 2, D_B2 = 3, D_OMB2 = 4, D_STEP = 5, D_BC2S = 6, D_EPS = 7;

__global__ void optim_set_k(double* __restrict__ h, double lr, double beta1, double beta2, double eps, double wd, double coupled) {
    h[0] = lr; h[1] = beta1; h[2] = beta2; h[3] = eps; h[4] = wd; h[5] = coupled; h[6] = 0.0; h[7] = 0.0;
}

// GUARD = true: `guard` is one `const double*`, the guard's state block; GUARD = false: an empty pack
template <bool GUARD, class... G>
__global__ __launch_bounds__(THREADS) void optim_advance_k(const hwgat_optim_entry* __restrict__ table, int n,
                                                           const double* __restrict__ hyper, float* __restrict__ derived,
                                                           G... guard) {
    if constexpr (GUARD) { if (gguard_skips(guard...)) return; }
    const int e = blockIdx.x * THREADS + threadIdx.x;
    if (e >= n) return;
    const hwgat_optim_entry en = table[e];
    const float t = *en.step + 1.0f;
    *en.step = t;
    const double* h = hyper + (int64_t)en.group * HWGAT_OPTIM_NHYPER;
    const double lr = h[0], b1 = h[1], b2 = h[2], eps = h[3], wd = h[4];
    const bool coupled = h[5] != 0.0;
    float* d = derived + (int64_t)e * HWGAT_OPTIM_NDERIVED;
    d[D_LRWD] = coupled ? 0.f : (float)(lr * wd);
    d[D_WD] = coupled ? (float)wd : 0.f;
    d[D_OMB1] = (float)(1.0 - b1);
    d[D_B2] = (float)b2;
    d[D_OMB2] = (float)(1.0 - b2);
    d[D_STEP] = (float)(lr / (1.0 - pow(b1, (double)t)));
    d[D_BC2S] = (float)sqrt(1.0 - pow(b2, (double)t));
    d[D_EPS] = (float)eps;
}

// the tensors' addresses come out of the table, so the compiler cannot tell that they are global memory and would issue
// flat loads and stores; said explicitly, they are global ones
typedef float __attribute__((address_space(1))) gfloat;
typedef f32x4 __attribute__((address_space(1))) gf32x4;

struct Scalars { float lrwd, wd, omb1, b2, omb2, step, bc2s, eps; };

// one element; the vector path and the scalar path share it, and contraction is off inside it, so which path an element
// takes (alignment, tail) cannot change its bits
__device__ __forceinline__ void adam1(const Scalars& s, float& p, float g, float& m, float& v) {
#pragma clang fp contract(off)
    p = fmaf(-s.lrwd, p, p);                                  // AdamW: p (1 - lr wd) in one rounding; Adam: lrwd = 0
    g = fmaf(s.wd, p, g);                                     // Adam: g + wd p; AdamW: wd = 0
    m = fmaf(s.omb1, g - m, m);
    v = fmaf(s.omb2 * g, g, s.b2 * v);
    const float denom = sqrtf(v) / s.bc2s + s.eps;
    p = fmaf(-s.step, m / denom, p);
}

template <bool GUARD, class... G>
__global__ __launch_bounds__(THREADS) void optim_step_k(const hwgat_optim_entry* __restrict__ table, int n,
                                                        const float* __restrict__ derived, G... guard) {
    if constexpr (GUARD) { if (gguard_skips(guard...)) return; }
    // entry of this workgroup: the last one whose first_block <= blockIdx.x.  Uniform binary search (a model has ~200
    // entries; the loads are scalar)
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (table[mid].first_block <= (int)blockIdx.x) lo = mid; else hi = mid - 1;
    }
    const hwgat_optim_entry en = table[lo];
    const float* d = derived + (int64_t)lo * HWGAT_OPTIM_NDERIVED;
    const Scalars s = {d[D_LRWD], d[D_WD], d[D_OMB1], d[D_B2], d[D_OMB2], d[D_STEP], d[D_BC2S], d[D_EPS]};
    const int64_t c0 = (int64_t)((int)blockIdx.x - en.first_block) * HWGAT_OPTIM_CHUNK;
    if (c0 >= en.n) return;                                   // cannot happen with a well-formed table
    const int count = (int)((en.n - c0 < HWGAT_OPTIM_CHUNK) ? en.n - c0 : HWGAT_OPTIM_CHUNK);
    gfloat* p = (gfloat*)en.p + c0;
    const gfloat* g = (const gfloat*)en.g + c0;
    gfloat* m = (gfloat*)en.m + c0;
    gfloat* v = (gfloat*)en.v + c0;
    // c0 is a multiple of 4 elements, so the chunk is 16-byte aligned exactly when the tensor is
    const bool aligned = ((((uintptr_t)en.p) | ((uintptr_t)en.g) | ((uintptr_t)en.m) | ((uintptr_t)en.v)) & 15) == 0;
    int done = 0;
    if (aligned) {
        const int nvec = count >> 2;
        // m, v and g are read once and (m, v) written once per step: nontemporal.  p is read again by the next step's
        // hwgat_weight_prep: plain
#pragma unroll
        for (int k = 0; k < VEC_PER_THREAD; ++k) {
            const int i = k * THREADS + threadIdx.x;
            if (i < nvec) {
                float pv[4], gv[4], mv[4], vv[4];
                const f32x4 pt = *(const gf32x4*)(p + i * 4);
                const f32x4 gt = __builtin_nontemporal_load((const gf32x4*)(g + i * 4));
                const f32x4 mt = __builtin_nontemporal_load((const gf32x4*)(m + i * 4));
                const f32x4 vt = __builtin_nontemporal_load((const gf32x4*)(v + i * 4));
#pragma unroll
                for (int j = 0; j < 4; ++j) { pv[j] = pt[j]; gv[j] = gt[j]; mv[j] = mt[j]; vv[j] = vt[j]; }
#pragma unroll
                for (int j = 0; j < 4; ++j) adam1(s, pv[j], gv[j], mv[j], vv[j]);
                *(gf32x4*)(p + i * 4) = f32x4{pv[0], pv[1], pv[2], pv[3]};
                __builtin_nontemporal_store(f32x4{mv[0], mv[1], mv[2], mv[3]}, (gf32x4*)(m + i * 4));
                __builtin_nontemporal_store(f32x4{vv[0], vv[1], vv[2], vv[3]}, (gf32x4*)(v + i * 4));
            }
        }
        done = nvec << 2;
    }
    // tails of aligned tensors (< 4 elements) and whole chunks of misaligned ones (gradients that are views into a flat
    // bucket: 4-byte aligned): one element per lane, still coalesced
    for (int i = done + threadIdx.x; i < count; i += THREADS) {
        float pe = p[i], me = m[i], ve = v[i];
        adam1(s, pe, g[i], me, ve);
        p[i] = pe; m[i] = me; v[i] = ve;
    }
}

}  // namespace

extern "C" int hwgat_optim_set(double* hyper, int group, double lr, double beta1, double beta2, double eps,
                               double weight_decay, int decoupled, void* stream) {
    if (!hyper || group < 0) return HWGAT_EINVAL;
    optim_set_k<<<1, 1, 0, (hipStream_t)stream>>>(hyper + (int64_t)group * HWGAT_OPTIM_NHYPER, lr, beta1, beta2, eps,
                                                  weight_decay, decoupled ? 0.0 : 1.0);
    HWGAT_LAUNCH_CHECK();
}

extern "C" int hwgat_optim_advance(const hwgat_optim_entry* table, int n, const double* hyper, float* derived, void* stream) {
    if (!table || !hyper || !derived || n <= 0) return HWGAT_EINVAL;
    optim_advance_k<false><<<(n + THREADS - 1) / THREADS, THREADS, 0, (hipStream_t)stream>>>(table, n, hyper, derived);
    HWGAT_LAUNCH_CHECK();
}

extern "C" int hwgat_optim_step(const hwgat_optim_entry* table, int n, const float* derived, int total_blocks, void* stream) {
    if (!table || !derived || n <= 0 || total_blocks <= 0) return HWGAT_EINVAL;
    optim_step_k<false><<<total_blocks, THREADS, 0, (hipStream_t)stream>>>(table, n, derived);
    HWGAT_LAUNCH_CHECK();
}

extern "C" int hwgat_gguard_adamw_advance(const hwgat_optim_entry* table, int n, const double* hyper, float* derived,
                                          const double* guard_state, void* stream) {
    if (!table || !hyper || !derived || !guard_state || n <= 0) return HWGAT_EINVAL;
    optim_advance_k<true><<<(n + THREADS - 1) / THREADS, THREADS, 0, (hipStream_t)stream>>>(table, n, hyper, derived, guard_state);
    HWGAT_LAUNCH_CHECK();
}

extern "C" int hwgat_gguard_adamw_step(const hwgat_optim_entry* table, int n, const float* derived, int total_blocks,
                                       const double* guard_state, void* stream) {
    if (!table || !derived || !guard_state || n <= 0 || total_blocks <= 0) return HWGAT_EINVAL;
    optim_step_k<true><<<total_blocks, THREADS, 0, (hipStream_t)stream>>>(table, n, derived, guard_state);
    HWGAT_LAUNCH_CHECK();
}
