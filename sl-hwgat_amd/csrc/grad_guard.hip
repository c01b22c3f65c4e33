// Gradient guard for gfx950 (wave64): the global norm of ALL gradients of a model, torch's clip coefficient from it, a
// "saw a NaN or an Inf" verdict and three counters, computed and kept on the device, and the in-place scaling of the
// gradients by that coefficient.  Table-driven like optim.hip: the launches read the optimizer's own table (only `g`, `n`
// and `first_block` of a record) and map workgroups to tensors as its step kernel does, so a train step captured in a HIP
// graph can hold them between its backward and its optimizer launches.
//
// Reference: torch.nn.utils.clip_grad_norm_(parameters, max_norm, norm_type = 2 | inf):
//     total_norm = || (||g_1||, ..., ||g_k||) ||        coef = clamp(max_norm / (total_norm + 1e-6), max = 1)
//     g_i *= coef
// Four kernels.  gguard_set_k writes the three config words from kernel arguments.  gguard_partial_k, one workgroup per
// chunk, leaves one fp64 partial (sum of squares, or max of magnitudes) and one flag word per workgroup in a workspace.
// gguard_finish_k, one workgroup, folds them and writes the state block.  gguard_scale_k streams the gradients once more.
//
// Determinism.  No atomics.  Every fp64 sum has one fixed shape: a thread adds its elements in ascending order of
// (k, j) -- vector k * 256 + thread of the chunk, element j of that vector --, the 64 lanes of a wave fold by a butterfly
// (xor 32, 16, ..., 1: every lane computes the same tree), the four waves fold as (w0 + w1) + (w2 + w3), and the finish
// kernel repeats that shape over the workgroups' partials (thread t takes t, t + 256, ...).  Which elements a thread
// takes depends on their index in the chunk only: a 16-byte-aligned tensor is read in 16-byte vectors, any other one
// element by element, and both hand thread t the same elements in the same order.  The norm therefore depends on the
// gradients' values and the tensors' sizes, not on where they lie.  g * g is exact in fp64 (24-bit significands).
#include <math.h>

#include "common.h"

namespace {

constexpr int THREADS = 256;
constexpr int WAVES = THREADS / HWGAT_WAVE;
constexpr int VEC_PER_THREAD = HWGAT_OPTIM_CHUNK / (THREADS * 4);
static_assert(VEC_PER_THREAD * THREADS * 4 == HWGAT_OPTIM_CHUNK, "a chunk is a whole number of 16-byte vectors per thread");
static_assert(HWGAT_GGUARD_SKIPPED < HWGAT_GGUARD_NSTATE, "the state block holds every slot");
constexpr int SAW_NAN = 1, SAW_INF = 2;

// the tensors' addresses come out of the table: said explicitly, they are global memory (global, not flat, accesses)
typedef float __attribute__((address_space(1))) gfloat;
typedef f32x4 __attribute__((address_space(1))) gf32x4;
typedef double f64x2 __attribute__((ext_vector_type(2)));

__global__ void gguard_set_k(double* __restrict__ state, double max_norm, double norm_type, double mode) {
    state[HWGAT_GGUARD_MAX_NORM] = max_norm;
    state[HWGAT_GGUARD_NORM_TYPE] = norm_type;
    state[HWGAT_GGUARD_MODE] = mode;
}

__device__ __forceinline__ double fold2(bool maxn, double a, double b) { return maxn ? fmax(a, b) : a + b; }

// one element into a thread's accumulator and flags.  fmax drops a NaN operand: the flag keeps it
__device__ __forceinline__ void take(bool maxn, float g, double& acc, int& flags) {
    const float a = fabsf(g);
    flags |= (a != a) ? SAW_NAN : (a == INFINITY ? SAW_INF : 0);
    acc = maxn ? fmax(acc, (double)a) : acc + (double)g * (double)g;
}

// (acc, flags) of the 256 threads folded into thread 0's: butterfly in each wave, then the four waves through LDS
__device__ __forceinline__ void fold_block(bool maxn, double& acc, int& flags) {
    __shared__ double s_acc[WAVES];
    __shared__ int s_flags[WAVES];
#pragma unroll
    for (int o = HWGAT_WAVE / 2; o > 0; o >>= 1) {
        acc = fold2(maxn, acc, __shfl_xor(acc, o, HWGAT_WAVE));
        flags |= __shfl_xor(flags, o, HWGAT_WAVE);
    }
    if (lane_id() == 0) {
        s_acc[threadIdx.x / HWGAT_WAVE] = acc;
        s_flags[threadIdx.x / HWGAT_WAVE] = flags;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        static_assert(WAVES == 4, "the fixed tree below is written for four waves");
        acc = fold2(maxn, fold2(maxn, s_acc[0], s_acc[1]), fold2(maxn, s_acc[2], s_acc[3]));
        flags = s_flags[0] | s_flags[1] | s_flags[2] | s_flags[3];
    }
}

__global__ __launch_bounds__(THREADS) void gguard_partial_k(const hwgat_opt_entry* __restrict__ table, int n,
                                                            const double* __restrict__ state,
                                                            double* __restrict__ workspace) {
    const bool maxn = state[HWGAT_GGUARD_NORM_TYPE] != 2.0;
    const hwgat_opt_entry en = table[entry_of_block(table, n)];
    const int64_t c0 = (int64_t)((int)blockIdx.x - en.first_block) * HWGAT_OPTIM_CHUNK;
    // c0 < n with a well-formed table; an empty chunk still writes its (neutral) partial, which the finish kernel reads
    const int count = c0 >= en.n ? 0 : (int)((en.n - c0 < HWGAT_OPTIM_CHUNK) ? en.n - c0 : HWGAT_OPTIM_CHUNK);
    const gfloat* g = (const gfloat*)en.g + c0;
    // c0 is a multiple of 4 elements, so the chunk is 16-byte aligned exactly when the tensor is
    const bool aligned = (((uintptr_t)en.g) & 15) == 0;
    double acc = 0.0;
    int flags = 0;
#pragma unroll
    for (int k = 0; k < VEC_PER_THREAD; ++k) {
        const int i = (k * THREADS + threadIdx.x) * 4;        // this thread's k-th vector: elements i .. i + 3
        if (aligned && i + 4 <= count) {
            const f32x4 gt = *(const gf32x4*)(g + i);         // plain: the scale and step kernels read g again
#pragma unroll
            for (int j = 0; j < 4; ++j) take(maxn, gt[j], acc, flags);
        } else {                                              // misaligned tensors, and the last (< 4) elements of any
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (i + j < count) take(maxn, g[i + j], acc, flags);
        }
    }
    fold_block(maxn, acc, flags);
    if (threadIdx.x == 0) *(f64x2*)(workspace + 2 * (int64_t)blockIdx.x) = f64x2{acc, (double)flags};
}

__global__ __launch_bounds__(THREADS) void gguard_finish_k(const double* __restrict__ workspace, int total_blocks,
                                                           double* __restrict__ state) {
    const bool maxn = state[HWGAT_GGUARD_NORM_TYPE] != 2.0;
    double acc = 0.0;
    int flags = 0;
    for (int b = threadIdx.x; b < total_blocks; b += THREADS) {
        const f64x2 w = *(const f64x2*)(workspace + 2 * (int64_t)b);
        acc = fold2(maxn, acc, w[0]);
        flags |= (int)w[1];
    }
    fold_block(maxn, acc, flags);
    if (threadIdx.x != 0) return;
    const bool nonfinite = flags != 0;
    const double total = maxn ? ((flags & SAW_NAN) ? (double)NAN : acc) : sqrt(acc);   // a sum carries its NaN / Inf itself
    const double c = state[HWGAT_GGUARD_MAX_NORM] / (total + 1e-6);
    const double coef = (c < 1.0 || c != c) ? c : 1.0;        // torch's clamp(max = 1) keeps a NaN
    const bool skip = nonfinite && state[HWGAT_GGUARD_MODE] != 0.0;
    state[HWGAT_GGUARD_TOTAL_NORM] = total;
    state[HWGAT_GGUARD_CLIP_COEF] = coef;
    state[HWGAT_GGUARD_NONFINITE] = nonfinite ? 1.0 : 0.0;
    state[HWGAT_GGUARD_SKIP] = skip ? 1.0 : 0.0;
    state[HWGAT_GGUARD_STEPS] += 1.0;
    if (coef < 1.0 && !skip) state[HWGAT_GGUARD_CLIPPED] += 1.0;
    if (skip) state[HWGAT_GGUARD_SKIPPED] += 1.0;
}

__global__ __launch_bounds__(THREADS) void gguard_scale_k(const hwgat_opt_entry* __restrict__ table, int n,
                                                          const double* __restrict__ state) {
    if (gguard_skips(state)) return;                          // the offending gradients stay as they are
    const float coef = (float)state[HWGAT_GGUARD_CLIP_COEF];
    const hwgat_opt_entry en = table[entry_of_block(table, n)];
    const int64_t c0 = (int64_t)((int)blockIdx.x - en.first_block) * HWGAT_OPTIM_CHUNK;
    if (c0 >= en.n) return;                                   // cannot happen with a well-formed table
    const int count = (int)((en.n - c0 < HWGAT_OPTIM_CHUNK) ? en.n - c0 : HWGAT_OPTIM_CHUNK);
    gfloat* g = (gfloat*)en.g + c0;
    int done = 0;
    if ((((uintptr_t)en.g) & 15) == 0) {
        const int nvec = count >> 2;
#pragma unroll
        for (int k = 0; k < VEC_PER_THREAD; ++k) {
            const int i = k * THREADS + threadIdx.x;
            if (i < nvec) *(gf32x4*)(g + i * 4) = *(const gf32x4*)(g + i * 4) * coef;   // plain: the step kernel reads g next
        }
        done = nvec << 2;
    }
    // tails of aligned tensors (< 4 elements) and whole chunks of misaligned ones: one element per lane, still coalesced
    for (int i = done + threadIdx.x; i < count; i += THREADS) g[i] = g[i] * coef;
}

}  // namespace

extern "C" int hwgat_gguard_set(double* state, double max_norm, double norm_type, int skip, void* stream) {
    if (!state || !(max_norm >= 0.0) || !(norm_type == 2.0 || norm_type == (double)INFINITY)) return HWGAT_EINVAL;
    gguard_set_k<<<1, 1, 0, (hipStream_t)stream>>>(state, max_norm, norm_type, skip ? 1.0 : 0.0);
    HWGAT_LAUNCH_CHECK();
}

extern "C" int hwgat_gguard_partial(const hwgat_opt_entry* table, int n, const double* state, double* workspace,
                                    int total_blocks, void* stream) {
    if (!table || !state || !workspace || (((uintptr_t)workspace) & 15) || n <= 0 || total_blocks <= 0) return HWGAT_EINVAL;
    gguard_partial_k<<<total_blocks, THREADS, 0, (hipStream_t)stream>>>(table, n, state, workspace);
    HWGAT_LAUNCH_CHECK();
}

extern "C" int hwgat_gguard_finish(const double* workspace, int total_blocks, double* state, void* stream) {
    if (!workspace || (((uintptr_t)workspace) & 15) || !state || total_blocks <= 0) return HWGAT_EINVAL;
    gguard_finish_k<<<1, THREADS, 0, (hipStream_t)stream>>>(workspace, total_blocks, state);
    HWGAT_LAUNCH_CHECK();
}

extern "C" int hwgat_gguard_scale(const hwgat_opt_entry* table, int n, const double* state, int total_blocks, void* stream) {
    if (!table || !state || n <= 0 || total_blocks <= 0) return HWGAT_EINVAL;
    gguard_scale_k<<<total_blocks, THREADS, 0, (hipStream_t)stream>>>(table, n, state);
    HWGAT_LAUNCH_CHECK();
}
