// SGD and NAdam for every parameter tensor of a model in ONE launch each on gfx950: the two optimizer types of the
// reference (hwgat/utils.py:73-84: cfg.optimizer_type 'sgd' / 'nadam') that csrc/optim.hip does not cover, in the same
// form -- a table in device memory, hyper-parameters in fp64 device words that the kernels read when they run, so a train
// step captured in a HIP graph holds its optimizer under any learning-rate schedule.
//
// Reference: torch.optim.SGD and torch.optim.NAdam with maximize = False on fp32 tensors.
//   SGD     g' = g + wd p
//           momentum != 0:  buf = g' the first time THIS tensor is stepped, buf = momentum buf + (1 - dampening) g' after;
//                           d = g' + momentum buf (nesterov) | d = buf
//           momentum == 0:  d = g'  (no buffer is read or written)
//           p -= lr d
//   NAdam   t += 1; mu = b1 (1 - 0.5 0.96^(t md)); mu' = b1 (1 - 0.5 0.96^((t + 1) md)); mu_product *= mu
//           p -= (lr wd) p  (decoupled)  |  g += wd p
//           m = m + (1 - b1) (g - m);  v = b2 v + ((1 - b2) g) g;  denom = sqrt(v / (1 - b2^t)) + eps
//           p -= [lr (1 - mu) / (1 - mu_product)] g / denom + [lr mu' / (1 - mu_product mu')] m / denom
// Per optimizer three kernels, as in optim.hip: *_set_k writes one group's hyper-parameters from kernel arguments;
// *_advance_k, one thread per table entry, updates the tensor's own scalar state (SGD: the "stepped before" word; NAdam:
// step count and mu_product) and rounds the entry's fp32 scalars from fp64 once; *_step_k streams the arrays.  No float
// atomics, no reductions, no LDS: the result is a pure function of its inputs.
//
// With a gradient guard (grad_guard.hip) the advance and step kernels are instantiated a second time, GUARD = true, with
// the guard's state block as one more argument, and return at once when its `skip` word is set: SGD's "stepped" word,
// NAdam's step count and mu_product, the parameters and the state arrays all stay as they are.  The GUARD = false
// instantiations take no such argument and hold no trace of the guard: hwgat_{sgd,nadam}_{advance,step} launch those.
#include "common.h"

namespace {

constexpr int THREADS = 256;
constexpr int VEC_PER_THREAD = HWGAT_OPTIM_CHUNK / (THREADS * 4);
static_assert(VEC_PER_THREAD * THREADS * 4 == HWGAT_OPTIM_CHUNK, "a chunk is a whole number of 16-byte vectors per thread");
static_assert(sizeof(hwgat_opt_entry) == 64, "the host packs 64-byte records (sl-hwgat_amd/optim.py)");

// slots of an entry's derived block
constexpr int S_LR = 0, S_WD = 1, S_MOM = 2, S_OMD = 3, S_NESTEROV = 4, S_FIRST = 5, S_HASBUF = 6;
constexpr int N_LRWD = 0, N_WD = 1, N_OMB1 = 2, N_B2 = 3, N_OMB2 = 4, N_BC2 = 5, N_EPS = 6, N_CG = 7, N_CM = 8;
static_assert(S_HASBUF < HWGAT_OPT_NDERIVED && N_CM < HWGAT_OPT_NDERIVED, "the derived block holds every slot");

__global__ void sgd_set_k(double* __restrict__ h, double lr, double momentum, double dampening, double wd, double nesterov) {
    h[0] = lr; h[1] = momentum; h[2] = dampening; h[3] = wd; h[4] = nesterov; h[5] = 0.0; h[6] = 0.0; h[7] = 0.0;
}

__global__ void nadam_set_k(double* __restrict__ h, double lr, double beta1, double beta2, double eps, double wd,
                            double coupled, double momentum_decay) {
    h[0] = lr; h[1] = beta1; h[2] = beta2; h[3] = eps; h[4] = wd; h[5] = coupled; h[6] = momentum_decay; h[7] = 0.0;
}

template <bool GUARD, class... G>
__global__ __launch_bounds__(THREADS) void sgd_advance_k(const hwgat_opt_entry* __restrict__ table, int n,
                                                         const double* __restrict__ hyper, float* __restrict__ derived,
                                                         G... guard) {
    if constexpr (GUARD) { if (gguard_skips(guard...)) return; }
    const int e = blockIdx.x * THREADS + threadIdx.x;
    if (e >= n) return;
    const hwgat_opt_entry en = table[e];
    const double* h = hyper + (int64_t)en.group * HWGAT_OPTIM_NHYPER;
    const double lr = h[0], mom = h[1], damp = h[2], wd = h[3];
    const bool hasbuf = mom != 0.0 && en.s0 != nullptr && en.w0 != nullptr;
    bool first = false;
    if (hasbuf) {                                             // torch clones the gradient into a tensor's first buffer
        first = *en.w0 == 0.0f;
        *en.w0 = 1.0f;
    }
    float* d = derived + (int64_t)e * HWGAT_OPT_NDERIVED;
    d[S_LR] = (float)lr;
    d[S_WD] = (float)wd;
    d[S_MOM] = (float)mom;
    d[S_OMD] = (float)(1.0 - damp);
    d[S_NESTEROV] = h[4] != 0.0 ? 1.f : 0.f;
    d[S_FIRST] = first ? 1.f : 0.f;
    d[S_HASBUF] = hasbuf ? 1.f : 0.f;
}

template <bool GUARD, class... G>
__global__ __launch_bounds__(THREADS) void nadam_advance_k(const hwgat_opt_entry* __restrict__ table, int n,
                                                           const double* __restrict__ hyper, float* __restrict__ derived,
                                                         G... guard) {
    if constexpr (GUARD) { if (gguard_skips(guard...)) return; }
    const int e = blockIdx.x * THREADS + threadIdx.x;
    if (e >= n) return;
    const hwgat_opt_entry en = table[e];
    const float t = *en.w0 + 1.0f;
    *en.w0 = t;
    const double* h = hyper + (int64_t)en.group * HWGAT_OPTIM_NHYPER;
    const double lr = h[0], b1 = h[1], b2 = h[2], eps = h[3], wd = h[4], md = h[6];
    const bool coupled = h[5] != 0.0;
    const double mu = b1 * (1.0 - 0.5 * pow(0.96, (double)t * md));
    const double mu_next = b1 * (1.0 - 0.5 * pow(0.96, ((double)t + 1.0) * md));
    const float mp = (float)((double)*en.w1 * mu);            // torch's state["mu_product"] is an fp32 word: so is this
    *en.w1 = mp;
    float* d = derived + (int64_t)e * HWGAT_OPT_NDERIVED;
    d[N_LRWD] = coupled ? 0.f : (float)(lr * wd);
    d[N_WD] = coupled ? (float)wd : 0.f;
    d[N_OMB1] = (float)(1.0 - b1);
    d[N_B2] = (float)b2;
    d[N_OMB2] = (float)(1.0 - b2);
    d[N_BC2] = (float)(1.0 - pow(b2, (double)t));
    d[N_EPS] = (float)eps;
    d[N_CG] = (float)(lr * (1.0 - mu) / (1.0 - (double)mp));
    d[N_CM] = (float)(lr * mu_next / (1.0 - (double)mp * mu_next));
}

// the tensors' addresses come out of the table: said explicitly, they are global memory (global, not flat, accesses)
typedef float __attribute__((address_space(1))) gfloat;
typedef f32x4 __attribute__((address_space(1))) gf32x4;

struct SgdScalars { float lr, wd, mom, omd; bool nesterov, first; };
struct NadamScalars { float lrwd, wd, omb1, b2, omb2, bc2, eps, cg, cm; };

// one element each; the vector path and the element path share them, and contraction is off inside them, so which path
// an element takes (alignment, tail) cannot change its bits
__device__ __forceinline__ void sgd_plain1(const SgdScalars& s, float& p, float g) {
#pragma clang fp contract(off)
    g = fmaf(s.wd, p, g);
    p = fmaf(-s.lr, g, p);
}

__device__ __forceinline__ void sgd_momentum1(const SgdScalars& s, float& p, float g, float& buf) {
#pragma clang fp contract(off)
    g = fmaf(s.wd, p, g);
    buf = s.first ? g : fmaf(s.omd, g, s.mom * buf);          // a select: what the buffer held before its first step is never used
    const float d = s.nesterov ? fmaf(s.mom, buf, g) : buf;
    p = fmaf(-s.lr, d, p);
}

__device__ __forceinline__ void nadam1(const NadamScalars& s, float& p, float g, float& m, float& v) {
#pragma clang fp contract(off)
    p = fmaf(-s.lrwd, p, p);                                  // decoupled: p (1 - lr wd) in one rounding; coupled: lrwd = 0
    g = fmaf(s.wd, p, g);                                     // coupled: g + wd p; decoupled: wd = 0
    m = fmaf(s.omb1, g - m, m);
    v = fmaf(s.omb2 * g, g, s.b2 * v);
    const float denom = sqrtf(v / s.bc2) + s.eps;
    p = fmaf(-s.cg, g / denom, p);
    p = fmaf(-s.cm, m / denom, p);
}

// one chunk of p, g and NS state arrays through f(p, g, a, b): 16-byte vectors when `aligned`, then (tails of aligned
// tensors, whole chunks of misaligned ones) one element per lane.  g and the state arrays are touched once per step:
// nontemporal.  p is read again by the next step's hwgat_weight_prep: plain
template <int NS, class F>
__device__ __forceinline__ void stream_chunk(gfloat* p, const gfloat* g, gfloat* a, gfloat* b, int count, bool aligned,
                                             const F& f) {
    int done = 0;
    if (aligned) {
        const int nvec = count >> 2;
#pragma unroll
        for (int k = 0; k < VEC_PER_THREAD; ++k) {
            const int i = k * THREADS + threadIdx.x;
            if (i < nvec) {
                float pv[4], gv[4], av[4] = {0.f, 0.f, 0.f, 0.f}, bv[4] = {0.f, 0.f, 0.f, 0.f};
                const f32x4 pt = *(const gf32x4*)(p + i * 4);
                const f32x4 gt = __builtin_nontemporal_load((const gf32x4*)(g + i * 4));
#pragma unroll
                for (int j = 0; j < 4; ++j) { pv[j] = pt[j]; gv[j] = gt[j]; }
                if constexpr (NS >= 1) {
                    const f32x4 at = __builtin_nontemporal_load((const gf32x4*)(a + i * 4));
#pragma unroll
                    for (int j = 0; j < 4; ++j) av[j] = at[j];
                }
                if constexpr (NS >= 2) {
                    const f32x4 bt = __builtin_nontemporal_load((const gf32x4*)(b + i * 4));
#pragma unroll
                    for (int j = 0; j < 4; ++j) bv[j] = bt[j];
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) f(pv[j], gv[j], av[j], bv[j]);
                *(gf32x4*)(p + i * 4) = f32x4{pv[0], pv[1], pv[2], pv[3]};
                if constexpr (NS >= 1) __builtin_nontemporal_store(f32x4{av[0], av[1], av[2], av[3]}, (gf32x4*)(a + i * 4));
                if constexpr (NS >= 2) __builtin_nontemporal_store(f32x4{bv[0], bv[1], bv[2], bv[3]}, (gf32x4*)(b + i * 4));
            }
        }
        done = nvec << 2;
    }
    for (int i = done + threadIdx.x; i < count; i += THREADS) {
        float pe = p[i], ae = 0.f, be = 0.f;
        if constexpr (NS >= 1) ae = a[i];
        if constexpr (NS >= 2) be = b[i];
        f(pe, g[i], ae, be);
        p[i] = pe;
        if constexpr (NS >= 1) a[i] = ae;
        if constexpr (NS >= 2) b[i] = be;
    }
}

template <bool GUARD, class... G>
__global__ __launch_bounds__(THREADS) void sgd_step_k(const hwgat_opt_entry* __restrict__ table, int n,
                                                      const float* __restrict__ derived, G... guard) {
    if constexpr (GUARD) { if (gguard_skips(guard...)) return; }
    const int e = entry_of_block(table, n);
    const hwgat_opt_entry en = table[e];
    const float* d = derived + (int64_t)e * HWGAT_OPT_NDERIVED;
    const SgdScalars s = {d[S_LR], d[S_WD], d[S_MOM], d[S_OMD], d[S_NESTEROV] != 0.f, d[S_FIRST] != 0.f};
    const bool hasbuf = d[S_HASBUF] != 0.f && en.s0 != nullptr;
    const int64_t c0 = (int64_t)((int)blockIdx.x - en.first_block) * HWGAT_OPTIM_CHUNK;
    if (c0 >= en.n) return;                                   // cannot happen with a well-formed table
    const int count = (int)((en.n - c0 < HWGAT_OPTIM_CHUNK) ? en.n - c0 : HWGAT_OPTIM_CHUNK);
    gfloat* p = (gfloat*)en.p + c0;
    const gfloat* g = (const gfloat*)en.g + c0;
    // c0 is a multiple of 4 elements, so the chunk is 16-byte aligned exactly when the tensor is
    if (hasbuf) {
        const bool aligned = ((((uintptr_t)en.p) | ((uintptr_t)en.g) | ((uintptr_t)en.s0)) & 15) == 0;
        stream_chunk<1>(p, g, (gfloat*)en.s0 + c0, (gfloat*)nullptr, count, aligned,
                        [&](float& pe, float ge, float& buf, float&) { sgd_momentum1(s, pe, ge, buf); });
    } else {
        const bool aligned = ((((uintptr_t)en.p) | ((uintptr_t)en.g)) & 15) == 0;
        stream_chunk<0>(p, g, (gfloat*)nullptr, (gfloat*)nullptr, count, aligned,
                        [&](float& pe, float ge, float&, float&) { sgd_plain1(s, pe, ge); });
    }
}

template <bool GUARD, class... G>
__global__ __launch_bounds__(THREADS) void nadam_step_k(const hwgat_opt_entry* __restrict__ table, int n,
                                                        const float* __restrict__ derived, G... guard) {
    if constexpr (GUARD) { if (gguard_skips(guard...)) return; }
    const int e = entry_of_block(table, n);
    const hwgat_opt_entry en = table[e];
    const float* d = derived + (int64_t)e * HWGAT_OPT_NDERIVED;
    const NadamScalars s = {d[N_LRWD], d[N_WD], d[N_OMB1], d[N_B2], d[N_OMB2], d[N_BC2], d[N_EPS], d[N_CG], d[N_CM]};
    const int64_t c0 = (int64_t)((int)blockIdx.x - en.first_block) * HWGAT_OPTIM_CHUNK;
    if (c0 >= en.n) return;                                   // cannot happen with a well-formed table
    const int count = (int)((en.n - c0 < HWGAT_OPTIM_CHUNK) ? en.n - c0 : HWGAT_OPTIM_CHUNK);
    const bool aligned = ((((uintptr_t)en.p) | ((uintptr_t)en.g) | ((uintptr_t)en.s0) | ((uintptr_t)en.s1)) & 15) == 0;
    stream_chunk<2>((gfloat*)en.p + c0, (const gfloat*)en.g + c0, (gfloat*)en.s0 + c0, (gfloat*)en.s1 + c0, count, aligned,
                    [&](float& pe, float ge, float& m, float& v) { nadam1(s, pe, ge, m, v); });
}

}  // namespace

extern "C" int hwgat_sgd_set(double* hyper, int group, double lr, double momentum, double dampening, double weight_decay,
                             int nesterov, void* stream) {
    if (!hyper || group < 0) return HWGAT_EINVAL;
    sgd_set_k<<<1, 1, 0, (hipStream_t)stream>>>(hyper + (int64_t)group * HWGAT_OPTIM_NHYPER, lr, momentum, dampening,
                                                weight_decay, nesterov ? 1.0 : 0.0);
    HWGAT_LAUNCH_CHECK();
}

extern "C" int hwgat_sgd_advance(const hwgat_opt_entry* table, int n, const double* hyper, float* derived, void* stream) {
    if (!table || !hyper || !derived || n <= 0) return HWGAT_EINVAL;
    sgd_advance_k<false><<<(n + THREADS - 1) / THREADS, THREADS, 0, (hipStream_t)stream>>>(table, n, hyper, derived);
    HWGAT_LAUNCH_CHECK();
}

extern "C" int hwgat_sgd_step(const hwgat_opt_entry* table, int n, const float* derived, int total_blocks, void* stream) {
    if (!table || !derived || n <= 0 || total_blocks <= 0) return HWGAT_EINVAL;
    sgd_step_k<false><<<total_blocks, THREADS, 0, (hipStream_t)stream>>>(table, n, derived);
    HWGAT_LAUNCH_CHECK();
}

extern "C" int hwgat_nadam_set(double* hyper, int group, double lr, double beta1, double beta2, double eps,
                               double weight_decay, double momentum_decay, int decoupled, void* stream) {
    if (!hyper || group < 0) return HWGAT_EINVAL;
    nadam_set_k<<<1, 1, 0, (hipStream_t)stream>>>(hyper + (int64_t)group * HWGAT_OPTIM_NHYPER, lr, beta1, beta2, eps,
                                                  weight_decay, decoupled ? 0.0 : 1.0, momentum_decay);
    HWGAT_LAUNCH_CHECK();
}

extern "C" int hwgat_nadam_advance(const hwgat_opt_entry* table, int n, const double* hyper, float* derived, void* stream) {
    if (!table || !hyper || !derived || n <= 0) return HWGAT_EINVAL;
    nadam_advance_k<false><<<(n + THREADS - 1) / THREADS, THREADS, 0, (hipStream_t)stream>>>(table, n, hyper, derived);
    HWGAT_LAUNCH_CHECK();
}

extern "C" int hwgat_nadam_step(const hwgat_opt_entry* table, int n, const float* derived, int total_blocks, void* stream) {
    if (!table || !derived || n <= 0 || total_blocks <= 0) return HWGAT_EINVAL;
    nadam_step_k<false><<<total_blocks, THREADS, 0, (hipStream_t)stream>>>(table, n, derived);
    HWGAT_LAUNCH_CHECK();
}

// the same launches under a gradient guard (grad_guard.hip): `guard_state` is the guard's HWGAT_GGUARD_NSTATE fp64 words
#define HWGAT_GUARDED_PAIR(kind)                                                                                          \
    extern "C" int hwgat_gguard_##kind##_advance(const hwgat_opt_entry* table, int n, const double* hyper, float* derived, \
                                                 const double* guard_state, void* stream) {                               \
        if (!table || !hyper || !derived || !guard_state || n <= 0) return HWGAT_EINVAL;                                  \
        kind##_advance_k<true><<<(n + THREADS - 1) / THREADS, THREADS, 0, (hipStream_t)stream>>>(table, n, hyper, derived, \
                                                                                                  guard_state);           \
        HWGAT_LAUNCH_CHECK();                                                                                             \
    }                                                                                                                     \
    extern "C" int hwgat_gguard_##kind##_step(const hwgat_opt_entry* table, int n, const float* derived, int total_blocks, \
                                              const double* guard_state, void* stream) {                                  \
        if (!table || !derived || !guard_state || n <= 0 || total_blocks <= 0) return HWGAT_EINVAL;                       \
        kind##_step_k<true><<<total_blocks, THREADS, 0, (hipStream_t)stream>>>(table, n, derived, guard_state);           \
        HWGAT_LAUNCH_CHECK();                                                                                             \
    }
HWGAT_GUARDED_PAIR(sgd)
HWGAT_GUARDED_PAIR(nadam)
#undef HWGAT_GUARDED_PAIR
