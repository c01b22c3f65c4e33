// Train meters for gfx950: the per-epoch numbers a training loop reports (reference hwgat/utils.py:109-114 reads
// `loss.item()` and the correct predictions back after every batch) summed on the device by one more launch behind the
// optimizer's, so that a train step captured in a HIP graph needs no host read per batch.  One block of device memory
// (layout: include/hwgat_hip.h, "train meters"): a header, the running words of the open epoch, a ring of per-step records
// and the closed epochs.
//
// Two kernels.  meter_fold_k, one thread, adds one step: integer counts, the loss in fp64 by ONE addition per step in
// fold order (what Python's `total += loss.item()` computes: a float32 widens to a double exactly and the sum rounds once
// per step), the gradient guard's verdict and norm when there is a guard, and one log record.  meter_close_k copies the
// running words into the next history slot and zeroes them.  No atomics and no reduction anywhere: every word has one
// writer and every sum one order.  All stores are plain vector stores.
#include "common.h"

namespace {

static_assert(HWGAT_METER_R_MAX_GRAD_NORM < HWGAT_METER_NRUN, "the running words hold every slot");
static_assert(HWGAT_METER_OVERFLOW < HWGAT_METER_RUN, "the header ends where the running words begin");
static_assert(HWGAT_METER_LOG == HWGAT_METER_RUN + HWGAT_METER_NRUN, "the log follows the running words");

struct meter_record {
    float loss;
    int32_t correct, rows;
    float grad_norm;
};
static_assert(sizeof(meter_record) == 16, "a log record is two 8-byte words");

constexpr int CLOSE_THREADS = 64;
static_assert(HWGAT_METER_NRUN <= CLOSE_THREADS, "one thread per running word");

__device__ __forceinline__ int64_t f32_word(float v) { return (int64_t)(uint64_t)__float_as_uint(v); }
__device__ __forceinline__ float word_f32(int64_t w) { return __uint_as_float((uint32_t)(uint64_t)w); }

__global__ void meter_fold_k(int64_t* __restrict__ block, const float* __restrict__ loss_p, const int64_t* __restrict__ correct_p,
                             const int32_t* __restrict__ n_rows, int batch_rows, const double* __restrict__ guard,
                             int log_capacity) {
#pragma clang fp contract(off)
    int64_t* run = block + HWGAT_METER_RUN;
    const float loss = *loss_p;
    const int64_t correct = *correct_p;
    const int64_t rows = n_rows ? (int64_t)*n_rows : (int64_t)batch_rows;
    run[HWGAT_METER_R_STEPS] += 1;
    run[HWGAT_METER_R_ROWS] += rows;
    run[HWGAT_METER_R_CORRECT] += correct;
    // finite: the exponent field is not all ones (no dependence on how the compiler treats isfinite)
    const bool finite = (__float_as_uint(loss) & 0x7f800000u) != 0x7f800000u;
    if (finite) {
        const int64_t seen = run[HWGAT_METER_R_FINITE_STEPS];
        run[HWGAT_METER_R_FINITE_STEPS] = seen + 1;
        const double sum = __longlong_as_double(run[HWGAT_METER_R_LOSS_SUM]) + (double)loss;   // one addition, rounded once
        run[HWGAT_METER_R_LOSS_SUM] = __double_as_longlong(sum);
        const float top = word_f32(run[HWGAT_METER_R_MAX_LOSS]);
        if (seen == 0 || loss > top) run[HWGAT_METER_R_MAX_LOSS] = f32_word(loss);
    } else {
        run[HWGAT_METER_R_NONFINITE_LOSS] += 1;
    }
    run[HWGAT_METER_R_LAST_LOSS] = f32_word(loss);
    float norm32 = 0.0f;
    if (guard) {
        if (gguard_skips(guard)) run[HWGAT_METER_R_SKIPPED] += 1;
        const double norm = guard[HWGAT_GGUARD_TOTAL_NORM];
        if (norm > __longlong_as_double(run[HWGAT_METER_R_MAX_GRAD_NORM]))                   // false for a NaN norm
            run[HWGAT_METER_R_MAX_GRAD_NORM] = __double_as_longlong(norm);
        norm32 = (float)norm;
    }
    if (log_capacity > 0) {
        const int64_t total = block[HWGAT_METER_LOG_TOTAL];
        meter_record rec;
        rec.loss = loss;
        rec.correct = (int32_t)correct;
        rec.rows = (int32_t)rows;
        rec.grad_norm = norm32;
        ((meter_record*)(block + HWGAT_METER_LOG))[total % log_capacity] = rec;
        block[HWGAT_METER_LOG_TOTAL] = total + 1;
    }
}

__global__ __launch_bounds__(CLOSE_THREADS) void meter_close_k(int64_t* __restrict__ block, int log_capacity, int history_capacity) {
    const int64_t closed = block[HWGAT_METER_CLOSED];
    __syncthreads();                                          // every thread has the count before thread 0 moves it
    int64_t* run = block + HWGAT_METER_RUN;
    const int t = threadIdx.x;
    if (t < HWGAT_METER_NRUN) {
        if (history_capacity > 0) {
            const int64_t slot = closed < history_capacity ? closed : history_capacity - 1;
            int64_t* hist = block + HWGAT_METER_LOG + 2 * (int64_t)log_capacity + slot * HWGAT_METER_NRUN;
            hist[t] = run[t];
        }
        run[t] = 0;
    }
    if (t == 0) {
        if (closed >= history_capacity) block[HWGAT_METER_OVERFLOW] += 1;
        block[HWGAT_METER_CLOSED] = closed + 1;
    }
}

bool capacities_ok(int log_capacity, int history_capacity) {
    return log_capacity >= 0 && history_capacity >= 0 && log_capacity <= HWGAT_METER_MAX_CAPACITY &&
           history_capacity <= HWGAT_METER_MAX_CAPACITY;
}

}  // namespace

extern "C" int64_t hwgat_meter_bytes(int log_capacity, int history_capacity) {
    if (!capacities_ok(log_capacity, history_capacity)) return HWGAT_EINVAL;
    return 8 * ((int64_t)HWGAT_METER_LOG + 2 * (int64_t)log_capacity + (int64_t)HWGAT_METER_NRUN * history_capacity);
}

extern "C" int hwgat_meter_fold(int64_t* block, const float* loss, const int64_t* correct, const int32_t* n_rows, int batch_rows,
                                const double* guard_state, int log_capacity, void* stream) {
    if (!block || (((uintptr_t)block) & 7) || !loss || !correct || (((uintptr_t)correct) & 7) || batch_rows < 0 ||
        !capacities_ok(log_capacity, 0))
        return HWGAT_EINVAL;
    meter_fold_k<<<1, 1, 0, (hipStream_t)stream>>>(block, loss, correct, n_rows, batch_rows, guard_state, log_capacity);
    HWGAT_LAUNCH_CHECK();
}

extern "C" int hwgat_meter_close(int64_t* block, int log_capacity, int history_capacity, void* stream) {
    if (!block || (((uintptr_t)block) & 7) || !capacities_ok(log_capacity, history_capacity)) return HWGAT_EINVAL;
    meter_close_k<<<1, CLOSE_THREADS, 0, (hipStream_t)stream>>>(block, log_capacity, history_capacity);
    HWGAT_LAUNCH_CHECK();
}
