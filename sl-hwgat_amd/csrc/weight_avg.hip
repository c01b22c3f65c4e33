// Weight averaging for gfx950 (wave64): an exponential moving average (EMA) or the equal-weight running mean (SWA) of every
// weight tensor of a model, kept on the device and updated by launches that a train step captured in a HIP graph holds after
// its optimizer launches.  Table-driven like optim.hip: one record per averaged tensor (hwgat_wavg_entry: the average, the
// live tensor, the element count, the first workgroup), one workgroup per HWGAT_OPTIM_CHUNK elements, and every number the
// update depends on in fp64 device words that the kernels read when they run.
//
// Reference: torch.optim.swa_utils.AveragedModel.update_parameters with get_ema_multi_avg_fn(decay) or the default
// (equal-weight) averaging function:
//     first update:   avg = p
//     EMA:            avg = avg + (1 - decay) (p - avg)            (torch: lerp(avg, p, 1 - decay))
//     equal weight:   avg = avg + (p - avg) / (n_averaged + 1)
// Four kernels.  wavg_set_k writes the five config words from kernel arguments.  wavg_advance_k, one thread, decides whether
// this step's update is due (a gradient guard that skipped the step: no; before `start` or off the `every` period: no) and
// leaves the verdict and the coefficient in the state block.  wavg_update_k streams avg and src once; wavg_swap_k
// exchanges them.  No atomics, no reductions: the result is a pure function of its inputs, and an element's bits do not
// depend on the path (vector, tail, misaligned) that moved it.
#include <math.h>

#include "common.h"

namespace {

constexpr int THREADS = 256;
constexpr int VEC_PER_THREAD = HWGAT_OPTIM_CHUNK / (THREADS * 4);
static_assert(VEC_PER_THREAD * THREADS * 4 == HWGAT_OPTIM_CHUNK, "a chunk is a whole number of 16-byte vectors per thread");
static_assert(sizeof(hwgat_wavg_entry) == HWGAT_WAVG_ENTRY_BYTES, "the host packs 32-byte records (sl-hwgat_amd/optim.py)");
static_assert(HWGAT_WAVG_ACTIVE < HWGAT_WAVG_NSTATE, "the state block holds every slot");

// the tensors' addresses come out of the table: said explicitly, they are global memory (global, not flat, accesses)
typedef float __attribute__((address_space(1))) gfloat;
typedef f32x4 __attribute__((address_space(1))) gf32x4;

__global__ void wavg_set_k(double* __restrict__ state, double mode, double decay, double warmup, double start, double every) {
    state[HWGAT_WAVG_MODE] = mode;
    state[HWGAT_WAVG_DECAY] = decay;
    state[HWGAT_WAVG_WARMUP] = warmup;
    state[HWGAT_WAVG_START] = start;
    state[HWGAT_WAVG_EVERY] = every;
}

// `guard` may be null: no gradient guard, every step counts
__global__ void wavg_advance_k(double* __restrict__ state, const double* __restrict__ guard) {
    if (guard && gguard_skips(guard)) {                       // the step did not happen: no counter moves
        state[HWGAT_WAVG_ACTIVE] = 0.0;
        state[HWGAT_WAVG_COEF] = 0.0;
        return;
    }
    const double seen = state[HWGAT_WAVG_STEPS_SEEN] + 1.0;
    state[HWGAT_WAVG_STEPS_SEEN] = seen;
    const double since = seen - state[HWGAT_WAVG_START];
    // counters and periods are whole numbers far below 2^53: fmod is exact
    if (!(since > 0.0 && fmod(since, state[HWGAT_WAVG_EVERY]) == 0.0)) {
        state[HWGAT_WAVG_ACTIVE] = 0.0;
        return;
    }
    const double k = state[HWGAT_WAVG_N_AVERAGED];
    double coef;
    if (k == 0.0) {
        coef = 1.0;                                           // the first update is a copy
    } else if (state[HWGAT_WAVG_MODE] == 0.0) {
        double d = state[HWGAT_WAVG_DECAY];
        if (state[HWGAT_WAVG_WARMUP] != 0.0) d = fmin(d, (1.0 + k) / (10.0 + k));
        coef = 1.0 - d;
    } else {
        coef = 1.0 / (k + 1.0);
    }
    state[HWGAT_WAVG_COEF] = coef;
    state[HWGAT_WAVG_N_AVERAGED] = k + 1.0;
    state[HWGAT_WAVG_ACTIVE] = 1.0;
}

// one element; the vector and the scalar path share it.  One subtraction and one fused multiply-add, each rounded once
__device__ __forceinline__ float avg1(float coef, float a, float p) {
#pragma clang fp contract(off)
    return fmaf(coef, p - a, a);
}

// this workgroup's chunk of its entry: the element count (0: nothing to do) and the two chunk pointers
__device__ __forceinline__ int chunk_of(const hwgat_wavg_entry& en, gfloat*& avg, gfloat*& src) {
    const int64_t c0 = (int64_t)((int)blockIdx.x - en.first_block) * HWGAT_OPTIM_CHUNK;
    if (c0 >= en.n) return 0;                                 // cannot happen with a well-formed table
    avg = (gfloat*)en.avg + c0;
    src = (gfloat*)en.src + c0;
    return (int)((en.n - c0 < HWGAT_OPTIM_CHUNK) ? en.n - c0 : HWGAT_OPTIM_CHUNK);
}

__global__ __launch_bounds__(THREADS) void wavg_update_k(const hwgat_wavg_entry* __restrict__ table, int n,
                                                         const double* __restrict__ state) {
    if (state[HWGAT_WAVG_ACTIVE] == 0.0) return;              // uniform, one scalar load: not due, or the step was skipped
    const double coef64 = state[HWGAT_WAVG_COEF];
    const bool copy = coef64 == 1.0;                          // the first update: the bits of src (also of a NaN, a -0)
    const float coef = (float)coef64;
    const hwgat_wavg_entry en = table[entry_of_block(table, n)];
    gfloat *avg, *src;
    const int count = chunk_of(en, avg, src);
    if (count == 0) return;
    int done = 0;
    // the chunk starts a multiple of 4 elements into the tensor, so it is 16-byte aligned exactly when the tensor is
    if (((((uintptr_t)en.avg) | ((uintptr_t)en.src)) & 15) == 0) {
        const int nvec = count >> 2;
        // avg is touched once per step: nontemporal.  src is read again by the next forward's weight prep: plain.  All of
        // a thread's loads are issued before the first use, so a wave has 2 * VEC_PER_THREAD vector loads in flight
        f32x4 pt[VEC_PER_THREAD], at[VEC_PER_THREAD];
#pragma unroll
        for (int k = 0; k < VEC_PER_THREAD; ++k) {
            const int i = k * THREADS + threadIdx.x;
            if (i < nvec) pt[k] = *(const gf32x4*)(src + i * 4);
        }
        if (!copy) {
#pragma unroll
            for (int k = 0; k < VEC_PER_THREAD; ++k) {
                const int i = k * THREADS + threadIdx.x;
                if (i < nvec) at[k] = __builtin_nontemporal_load((const gf32x4*)(avg + i * 4));
            }
        }
#pragma unroll
        for (int k = 0; k < VEC_PER_THREAD; ++k) {
            const int i = k * THREADS + threadIdx.x;
            if (i < nvec) {
                f32x4 out = pt[k];
                if (!copy) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) out[j] = avg1(coef, at[k][j], pt[k][j]);
                }
                __builtin_nontemporal_store(out, (gf32x4*)(avg + i * 4));
            }
        }
        done = nvec << 2;
    }
    // tails of aligned tensors (< 4 elements) and whole chunks of misaligned ones (views at any 4-byte offset of an arena):
    // one element per lane, still coalesced
    for (int i = done + threadIdx.x; i < count; i += THREADS) {
        const float p = src[i];
        avg[i] = copy ? p : avg1(coef, avg[i], p);
    }
}

__global__ __launch_bounds__(THREADS) void wavg_swap_k(const hwgat_wavg_entry* __restrict__ table, int n) {
    const hwgat_wavg_entry en = table[entry_of_block(table, n)];
    gfloat *avg, *src;
    const int count = chunk_of(en, avg, src);
    if (count == 0) return;
    int done = 0;
    if (((((uintptr_t)en.avg) | ((uintptr_t)en.src)) & 15) == 0) {
        const int nvec = count >> 2;
        f32x4 pt[VEC_PER_THREAD], at[VEC_PER_THREAD];
#pragma unroll
        for (int k = 0; k < VEC_PER_THREAD; ++k) {
            const int i = k * THREADS + threadIdx.x;
            if (i < nvec) {
                pt[k] = *(const gf32x4*)(src + i * 4);
                at[k] = __builtin_nontemporal_load((const gf32x4*)(avg + i * 4));
            }
        }
#pragma unroll
        for (int k = 0; k < VEC_PER_THREAD; ++k) {
            const int i = k * THREADS + threadIdx.x;
            if (i < nvec) {
                *(gf32x4*)(src + i * 4) = at[k];              // plain: the next forward reads it
                __builtin_nontemporal_store(pt[k], (gf32x4*)(avg + i * 4));
            }
        }
        done = nvec << 2;
    }
    for (int i = done + threadIdx.x; i < count; i += THREADS) {
        const float p = src[i], a = avg[i];
        src[i] = a;
        avg[i] = p;
    }
}

}  // namespace

extern "C" int hwgat_wavg_set(double* state, int mode, double decay, int warmup, int64_t start, int64_t every, void* stream) {
    if (!state || (mode != 0 && mode != 1) || !(decay >= 0.0 && decay < 1.0) || start < 0 || every < 1) return HWGAT_EINVAL;
    wavg_set_k<<<1, 1, 0, (hipStream_t)stream>>>(state, (double)mode, decay, warmup ? 1.0 : 0.0, (double)start, (double)every);
    HWGAT_LAUNCH_CHECK();
}

extern "C" int hwgat_wavg_advance(double* state, const double* guard_state, void* stream) {
    if (!state) return HWGAT_EINVAL;
    wavg_advance_k<<<1, 1, 0, (hipStream_t)stream>>>(state, guard_state);
    HWGAT_LAUNCH_CHECK();
}

extern "C" int hwgat_wavg_update(const hwgat_wavg_entry* table, int n, const double* state, int total_blocks, void* stream) {
    if (!table || (((uintptr_t)table) & 7) || !state || n <= 0 || total_blocks <= 0) return HWGAT_EINVAL;
    wavg_update_k<<<total_blocks, THREADS, 0, (hipStream_t)stream>>>(table, n, state);
    HWGAT_LAUNCH_CHECK();
}

extern "C" int hwgat_wavg_swap(const hwgat_wavg_entry* table, int n, int total_blocks, void* stream) {
    if (!table || (((uintptr_t)table) & 7) || n <= 0 || total_blocks <= 0) return HWGAT_EINVAL;
    wavg_swap_k<<<total_blocks, THREADS, 0, (hipStream_t)stream>>>(table, n);
    HWGAT_LAUNCH_CHECK();
}
