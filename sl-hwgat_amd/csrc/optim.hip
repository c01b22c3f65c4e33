// AdamW / Adam, SGD and NAdam for every parameter tensor of a model in ONE launch each on gfx950: the optimizer types of
// the reference (hwgat/utils.py:71-84: cfg.optimizer_type 'adamw' / 'adam' / 'sgd' / 'nadam'), driven by a table in device
// memory (the idiom of hwgat_weight_prep, prep.hip), with every hyper-parameter in fp64 device words that the kernels read
// when they run (the idiom of the dropout seed, embed.hip: hwgat_seed_set / hwgat_seed_advance).  A train step captured
// in a HIP graph can therefore hold its optimizer: a new learning rate reaches a replay through hwgat_opt_set, a launch of
// its own outside the graph, and nothing of the step is frozen at capture.
//
// Reference: torch.optim.AdamW / Adam (amsgrad off), torch.optim.SGD and torch.optim.NAdam with maximize = False on fp32
// parameters, gradients and state.
//   AdamW   p *= 1 - lr wd   (AdamW)    |    g += wd p   (Adam)
//           m  = m + (1 - b1) (g - m)
//           v  = b2 v + (1 - b2) g g
//           p -= (lr / (1 - b1^t)) m / (sqrt(v) / sqrt(1 - b2^t) + eps)
//   SGD     g' = g + wd p
//           momentum != 0:  buf = g' the first time THIS tensor is stepped, buf = momentum buf + (1 - dampening) g' after;
//                           d = g' + momentum buf (nesterov) | d = buf
//           momentum == 0:  d = g'  (no buffer is read or written)
//           p -= lr d
//   NAdam   t += 1; mu = b1 (1 - 0.5 0.96^(t md)); mu' = b1 (1 - 0.5 0.96^((t + 1) md)); mu_product *= mu
//           p -= (lr wd) p  (decoupled)  |  g += wd p
//           m = m + (1 - b1) (g - m);  v = b2 v + ((1 - b2) g) g;  denom = sqrt(v / (1 - b2^t)) + eps
//           p -= [lr (1 - mu) / (1 - mu_product)] g / denom + [lr mu' / (1 - mu_product mu')] m / denom
// opt_set_k, one thread, writes one group's hyper-parameters from a kernel argument.  Per optimizer two kernels:
// *_advance_k, one thread per table entry, updates the tensor's own scalar state (AdamW: the step count; SGD: the "stepped
// before" word; NAdam: step count and mu_product) and rounds the entry's fp32 scalars from fp64 once (the pow() and the
// divisions are done once per tensor, not once per workgroup); *_step_k streams the arrays through stream_chunk.  No float
// atomics, no reductions, no LDS: the result is a pure function of its inputs.
//
// With a gradient guard (grad_guard.hip) the advance and step kernels are instantiated a second time, GUARD = true, with
// the guard's state block as one more argument, and return at once when its `skip` word is set: a step whose gradients
// hold a NaN or an Inf changes no step count, "stepped" word or mu_product, no parameter and no state array.  The
// GUARD = false instantiations take no such argument and hold no trace of the guard; hwgat_opt_advance and hwgat_opt_step
// launch the one or the other by whether they are given a guard.
#include "common.h"

namespace {

constexpr int THREADS = 256;
constexpr int VEC_PER_THREAD = HWGAT_OPTIM_CHUNK / (THREADS * 4);
static_assert(VEC_PER_THREAD * THREADS * 4 == HWGAT_OPTIM_CHUNK, "a chunk is a whole number of 16-byte vectors per thread");
static_assert(sizeof(hwgat_opt_entry) == 64, "the host packs 64-byte records (sl-hwgat_amd/optim.py)");

// slots of an entry's derived block
constexpr int A_LRWD = 0, A_WD = 1, A_OMB1 = 2, A_B2 = 3, A_OMB2 = 4, A_STEP = 5, A_BC2S = 6, A_EPS = 7;
constexpr int S_LR = 0, S_WD = 1, S_MOM = 2, S_OMD = 3, S_NESTEROV = 4, S_FIRST = 5, S_HASBUF = 6;
constexpr int N_LRWD = 0, N_WD = 1, N_OMB1 = 2, N_B2 = 3, N_OMB2 = 4, N_BC2 = 5, N_EPS = 6, N_CG = 7, N_CM = 8;
static_assert(A_EPS < HWGAT_OPT_NDERIVED && S_HASBUF < HWGAT_OPT_NDERIVED && N_CM < HWGAT_OPT_NDERIVED,
              "the derived block holds every slot");

// a group's HWGAT_OPTIM_NHYPER words as one kernel argument: they travel with the launch, the host buffer is done with
struct HyperWords { double w[HWGAT_OPTIM_NHYPER]; };

__global__ void opt_set_k(double* __restrict__ h, HyperWords v) {
#pragma unroll
    for (int i = 0; i < HWGAT_OPTIM_NHYPER; ++i) h[i] = v.w[i];
}

// GUARD = true: `guard` is one `const double*`, the guard's state block; GUARD = false: an empty pack
template <bool GUARD, class... G>
__global__ __launch_bounds__(THREADS) void adamw_advance_k(const hwgat_opt_entry* __restrict__ table, int n,
                                                           const double* __restrict__ hyper, float* __restrict__ derived,
                                                           G... guard) {
    if constexpr (GUARD) { if (gguard_skips(guard...)) return; }
    const int e = blockIdx.x * THREADS + threadIdx.x;
    if (e >= n) return;
    const hwgat_opt_entry en = table[e];
    const float t = *en.w0 + 1.0f;
    *en.w0 = t;
    const double* h = hyper + (int64_t)en.group * HWGAT_OPTIM_NHYPER;
    const double lr = h[0], b1 = h[1], b2 = h[2], eps = h[3], wd = h[4];
    const bool coupled = h[5] != 0.0;
    float* d = derived + (int64_t)e * HWGAT_OPT_NDERIVED;
    d[A_LRWD] = coupled ? 0.f : (float)(lr * wd);
    d[A_WD] = coupled ? (float)wd : 0.f;
    d[A_OMB1] = (float)(1.0 - b1);
    d[A_B2] = (float)b2;
    d[A_OMB2] = (float)(1.0 - b2);
    d[A_STEP] = (float)(lr / (1.0 - pow(b1, (double)t)));
    d[A_BC2S] = (float)sqrt(1.0 - pow(b2, (double)t));
    d[A_EPS] = (float)eps;
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

struct AdamScalars { float lrwd, wd, omb1, b2, omb2, step, bc2s, eps; };
struct SgdScalars { float lr, wd, mom, omd; bool nesterov, first; };
struct NadamScalars { float lrwd, wd, omb1, b2, omb2, bc2, eps, cg, cm; };

// one element each; the vector path and the element path share them, and contraction is off inside them, so which path
// an element takes (alignment, tail) cannot change its bits
__device__ __forceinline__ void adam1(const AdamScalars& s, float& p, float g, float& m, float& v) {
#pragma clang fp contract(off)
    p = fmaf(-s.lrwd, p, p);                                  // AdamW: p (1 - lr wd) in one rounding; Adam: lrwd = 0
    g = fmaf(s.wd, p, g);                                     // Adam: g + wd p; AdamW: wd = 0
    m = fmaf(s.omb1, g - m, m);
    v = fmaf(s.omb2 * g, g, s.b2 * v);
    const float denom = sqrtf(v) / s.bc2s + s.eps;
    p = fmaf(-s.step, m / denom, p);
}

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
__global__ __launch_bounds__(THREADS) void adamw_step_k(const hwgat_opt_entry* __restrict__ table, int n,
                                                        const float* __restrict__ derived, G... guard) {
    if constexpr (GUARD) { if (gguard_skips(guard...)) return; }
    const int e = entry_of_block(table, n);
    const hwgat_opt_entry en = table[e];
    const float* d = derived + (int64_t)e * HWGAT_OPT_NDERIVED;
    const AdamScalars s = {d[A_LRWD], d[A_WD], d[A_OMB1], d[A_B2], d[A_OMB2], d[A_STEP], d[A_BC2S], d[A_EPS]};
    const int64_t c0 = (int64_t)((int)blockIdx.x - en.first_block) * HWGAT_OPTIM_CHUNK;
    if (c0 >= en.n) return;                                   // cannot happen with a well-formed table
    const int count = (int)((en.n - c0 < HWGAT_OPTIM_CHUNK) ? en.n - c0 : HWGAT_OPTIM_CHUNK);
    // c0 is a multiple of 4 elements, so the chunk is 16-byte aligned exactly when the tensor is
    const bool aligned = ((((uintptr_t)en.p) | ((uintptr_t)en.g) | ((uintptr_t)en.s0) | ((uintptr_t)en.s1)) & 15) == 0;
    stream_chunk<2>((gfloat*)en.p + c0, (const gfloat*)en.g + c0, (gfloat*)en.s0 + c0, (gfloat*)en.s1 + c0, count, aligned,
                    [&](float& pe, float ge, float& m, float& v) { adam1(s, pe, ge, m, v); });
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

// the advance / step launch of `kind`, GUARD = true with the guard's state block as `guard`
template <bool GUARD, class... G>
int launch_advance(int kind, const hwgat_opt_entry* table, int n, const double* hyper, float* derived, hipStream_t st,
                   G... guard) {
    const int blocks = (n + THREADS - 1) / THREADS;
    switch (kind) {
        case HWGAT_OPT_ADAMW: adamw_advance_k<GUARD><<<blocks, THREADS, 0, st>>>(table, n, hyper, derived, guard...); break;
        case HWGAT_OPT_SGD: sgd_advance_k<GUARD><<<blocks, THREADS, 0, st>>>(table, n, hyper, derived, guard...); break;
        case HWGAT_OPT_NADAM: nadam_advance_k<GUARD><<<blocks, THREADS, 0, st>>>(table, n, hyper, derived, guard...); break;
        default: return HWGAT_EINVAL;
    }
    HWGAT_LAUNCH_CHECK();
}

template <bool GUARD, class... G>
int launch_step(int kind, const hwgat_opt_entry* table, int n, const float* derived, int total_blocks, hipStream_t st,
                G... guard) {
    switch (kind) {
        case HWGAT_OPT_ADAMW: adamw_step_k<GUARD><<<total_blocks, THREADS, 0, st>>>(table, n, derived, guard...); break;
        case HWGAT_OPT_SGD: sgd_step_k<GUARD><<<total_blocks, THREADS, 0, st>>>(table, n, derived, guard...); break;
        case HWGAT_OPT_NADAM: nadam_step_k<GUARD><<<total_blocks, THREADS, 0, st>>>(table, n, derived, guard...); break;
        default: return HWGAT_EINVAL;
    }
    HWGAT_LAUNCH_CHECK();
}

bool known_kind(int kind) { return kind == HWGAT_OPT_ADAMW || kind == HWGAT_OPT_SGD || kind == HWGAT_OPT_NADAM; }

}  // namespace

extern "C" int hwgat_opt_set(double* hyper, int group, int kind, const double* values, void* stream) {
    if (!hyper || !values || group < 0 || !known_kind(kind)) return HWGAT_EINVAL;
    HyperWords v;
    for (int i = 0; i < HWGAT_OPTIM_NHYPER; ++i) v.w[i] = values[i];
    opt_set_k<<<1, 1, 0, (hipStream_t)stream>>>(hyper + (int64_t)group * HWGAT_OPTIM_NHYPER, v);
    HWGAT_LAUNCH_CHECK();
}

extern "C" int hwgat_opt_advance(int kind, const hwgat_opt_entry* table, int n, const double* hyper, float* derived,
                                 const double* guard_state, void* stream) {
    if (!table || !hyper || !derived || n <= 0) return HWGAT_EINVAL;
    const hipStream_t st = (hipStream_t)stream;
    return guard_state ? launch_advance<true>(kind, table, n, hyper, derived, st, guard_state)
                       : launch_advance<false>(kind, table, n, hyper, derived, st);
}

extern "C" int hwgat_opt_step(int kind, const hwgat_opt_entry* table, int n, const float* derived, int total_blocks,
                              const double* guard_state, void* stream) {
    if (!table || !derived || n <= 0 || total_blocks <= 0) return HWGAT_EINVAL;
    const hipStream_t st = (hipStream_t)stream;
    return guard_state ? launch_step<true>(kind, table, n, derived, total_blocks, st, guard_state)
                       : launch_step<false>(kind, table, n, derived, total_blocks, st);
}
