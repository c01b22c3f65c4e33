// Streaming recognition for gfx950 (serve.StreamRecognizer): n_streams keypoint streams in device ring buffers.  A live
// recogniser receives one raw (J, C) frame at a time; keeping the last frames, cutting the window, EvalTransform.draw and the
// decision on the logits all needed the host before, around a forward of under a millisecond.  Three kernels put that on
// the device with every changing value in device words (layout: include/hwgat_hip.h, "streaming recognition"), so that
// push -> window -> hwgat_aug_hand_fill -> hwgat_aug_resample -> forward -> decide is one HIP graph:
//
//   stream_push_k    one workgroup per stream appends up to push_frames frames to its ring.
//   stream_window_k  one workgroup per stream: a one-wave prefix sum of the window lengths (n_streams <= 64) gives its offset
//                    in the packed clip; it copies its newest frames oldest first, writes the frame map of TemporalSample
//                    and the eval parameter record with NormalizeKeypoints' left_top / edge_dist in the reference's fp32.
//   stream_decide_k  one workgroup, a wave per stream: softmax, exponential smoothing, lowest arg-max, the run / hold /
//                    threshold rule; one thread appends the events to the shared log in stream order.
//
// These are latency kernels (a few KB each).  No float atomics and no cross-workgroup communication: every word has one
// writer per launch and every sum one order.  Every index formed from a device word (head, count, n_new, log_count) is
// reduced to its range before use.  All stores are plain vector stores.
#include <limits.h>
#include <math.h>

#include "common.h"
#include "linspace.h"

namespace {

static_assert(sizeof(hwgat_stream_header) == 64, "the header is 8 words");
static_assert(sizeof(hwgat_stream_words) == 64, "a stream's record is 8 words");
static_assert(sizeof(hwgat_stream_event) == 32, "an event is 4 words");
static_assert(HWGAT_STREAM_MAX_STREAMS <= 64, "the prefix sum of the window lengths is one wave");

constexpr int PUSH_THREADS = 256, WIN_THREADS = 256, DEC_THREADS = 1024, DEC_WAVES = DEC_THREADS / 64;
constexpr int STREAM_MAX_JOINTS = 1024;
constexpr int DEC_UNROLL = 8;                                 // row entries a lane of the decide kernel loads per trip

__device__ __forceinline__ hwgat_stream_words* words_of(void* state, int s) {
    return reinterpret_cast<hwgat_stream_words*>(static_cast<char*>(state) + sizeof(hwgat_stream_header)) + s;
}
__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }
// a head word, whatever it holds, as a slot of the ring
__device__ __forceinline__ int ring_slot(int v, int R) {
    const int m = v % R;
    return m < 0 ? m + R : m;
}

__global__ __launch_bounds__(PUSH_THREADS) void stream_push_k(float* __restrict__ ring, void* state,
                                                              const float* __restrict__ frames,
                                                              const int32_t* __restrict__ n_new, int R, int F, int JC) {
    const int s = blockIdx.x;
    hwgat_stream_words* w = words_of(state, s);
    const int head = ring_slot(w->head, R);
    const int count = clampi(w->count, 0, R);
    const int n = clampi(n_new[s], 0, F);
    __syncthreads();                                          // every thread has the words before thread 0 moves them
    const float* src = frames + (int64_t)s * F * JC;
    float* dst = ring + (int64_t)s * R * JC;
    for (int e = threadIdx.x; e < n * JC; e += PUSH_THREADS) {
        const int f = e / JC, r = e - f * JC;
        int slot = head + f;                                  // head < R and f < F <= R: one wrap at most
        if (slot >= R) slot -= R;
        dst[(int64_t)slot * JC + r] = src[e];
    }
    if (threadIdx.x == 0) {
        int h = head + n;
        if (h >= R) h -= R;
        w->head = h;
        w->count = min(count + n, R);
        w->frames_seen += n;
    }
}

__global__ __launch_bounds__(WIN_THREADS) void stream_window_k(const float* __restrict__ ring, void* state,
                                                               float* __restrict__ clip, int32_t* __restrict__ clip_off,
                                                               int32_t* __restrict__ src, double* __restrict__ prm, int S,
                                                               int R, int Wf, int min_frames, int n, int J, int C, int o,
                                                               int a0, int a1) {
    __shared__ int sh_off, sh_first;
    const int s = blockIdx.x, t = threadIdx.x;
    // the window lengths of all streams, summed by the first wave: this stream's offset in the packed clip
    if (t < 64) {
        const int Li = t < S ? min(clampi(words_of(state, t)->count, 0, R), Wf) : 0;
        int inc = Li;
        for (int d = 1; d < 64; d <<= 1) {
            const int up = __shfl_up(inc, d, 64);
            if (t >= d) inc += up;
        }
        if (t == s) {
            sh_off = inc - Li;
            clip_off[s] = inc - Li;
            if (s == S - 1) clip_off[S] = inc;
        }
        if (t == 0) sh_first = INT_MAX;
    }
    __syncthreads();
    hwgat_stream_words* w = words_of(state, s);
    const int head = ring_slot(w->head, R), count = clampi(w->count, 0, R);
    const int L = min(count, Wf), off = sh_off, JC = J * C;   // off + L <= S * Wf: every stream adds at most Wf
    int start = head - L;                                     // the oldest frame of the window; head < R, L <= R
    if (start < 0) start += R;
    const float* rs = ring + (int64_t)s * R * JC;
    float* cd = clip + (int64_t)off * JC;
    for (int e = t; e < L * JC; e += WIN_THREADS) {
        const int f = e / JC, r = e - f * JC;
        int slot = start + f;
        if (slot >= R) slot -= R;
        cd[e] = rs[(int64_t)slot * JC + r];
    }
    // NormalizeKeypoints: the first frame whose origin and anchors are non-zero in every coordinate (an integer minimum in
    // LDS: the same whatever the order)
    for (int f = t; f < L; f += WIN_THREADS) {
        int slot = start + f;
        if (slot >= R) slot -= R;
        const float* kp = rs + (int64_t)slot * JC;
        bool ok = true;
        for (int c = 0; c < C; ++c) ok = ok && kp[o * C + c] != 0.f && kp[a0 * C + c] != 0.f && kp[a1 * C + c] != 0.f;
        if (ok) atomicMin(&sh_first, f);
    }
    __syncthreads();
    const int first = sh_first;
    float lt0 = 0.f, lt1 = 0.f, lt2 = 0.f, edge = 1.f;
    bool found = false;
    if (first < L) {
        int slot = start + first;
        if (slot >= R) slot -= R;
        const float* kp = rs + (int64_t)slot * JC;
        // fp32 with every product, sum and difference rounded on its own, as numpy computes them
        float sq = 0.f;
        for (int c = 0; c < C; ++c) {
            const float d = __fsub_rn(kp[a0 * C + c], kp[a1 * C + c]);
            sq = __fadd_rn(sq, __fmul_rn(d, d));
        }
        const float unit = __fsqrt_rn(sq);
        if (unit > 0.f && unit < INFINITY) {
            found = true;
            const float u3 = __fmul_rn(3.f, unit);
            lt0 = __fsub_rn(kp[o * C], u3);
            lt1 = __fsub_rn(kp[o * C + 1], __fmul_rn(2.f, unit));
            if (C > 2) lt2 = __fsub_rn(kp[o * C + 2], u3);
            edge = __fmul_rn(6.f, unit);
        }
    }
    if (t < HWGAT_AUG_NPRM) {
        double v = 0.0;
        if (t == 0) v = (double)lt0;
        else if (t == 1) v = (double)lt1;
        else if (t == 2) v = (double)lt2;
        else if (t == 3) v = (double)edge;
        else if (t == 11 || t == 15 || t == 19) v = 1.0;      // M = I
        else if (t == 21) v = L <= n ? 1.0 : 0.0;             // TemporalSample padded the clip
        prm[(int64_t)s * HWGAT_AUG_NPRM + t] = v;
    }
    // TemporalSample(random_shift = False) as a frame map
    for (int i = t; i < n; i += WIN_THREADS) {
        int m = 0;
        if (L > 0 && L <= n) {
            const int st = (n - L) / 2;
            m = (i >= st && i < st + L) ? i - st : (i < n / 2 ? 0 : L - 1);
        } else if (L > n && n > 1) {
            // numpy.linspace(0, L - 1, n).astype(int): arange(n) * ((L - 1) / (n - 1)) in fp64, the last entry L - 1
            m = linspace_int(i, L - 1, n);
        }
        src[(int64_t)s * n + i] = m;
    }
    if (t == 0) {
        w->ready = (found && count >= min_frames) ? 1 : 0;
        w->win_len = L;
    }
}

__global__ __launch_bounds__(DEC_THREADS) void stream_decide_k(void* state, float* __restrict__ q,
                                                               const float* __restrict__ logits, int S, int N,
                                                               int log_capacity) {
    __shared__ int sh_emit[HWGAT_STREAM_MAX_STREAMS], sh_top[HWGAT_STREAM_MAX_STREAMS];
    __shared__ float sh_conf[HWGAT_STREAM_MAX_STREAMS];
    __shared__ int64_t sh_eval[HWGAT_STREAM_MAX_STREAMS];
    hwgat_stream_header* hd = static_cast<hwgat_stream_header*>(state);
    const float alpha = hd->alpha, thr = hd->threshold;
    const float keep = __fsub_rn(1.f, alpha);
    const int hold = max(hd->hold, 1), blank = hd->blank_class;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int s = wave; s < S; s += DEC_WAVES) {               // uniform in a wave
        hwgat_stream_words* w = words_of(state, s);
        const bool ready = w->ready != 0;
        const int64_t evals = w->evals;
        bool emit = false;
        int top = 0;
        float conf = 0.f;
        if (ready) {
            const float* z = logits + (int64_t)s * N;
            float* qs = q + (int64_t)s * N;
            // a lane walks its entries (lane, lane + 64, ..) in ascending order, DEC_UNROLL of them per trip with the loads
            // issued together: a row is a few KB and the walk is latency, one load per trip would wait for each in turn
            float mx = -INFINITY;
            for (int i0 = lane; i0 < N; i0 += 64 * DEC_UNROLL) {
                float zv[DEC_UNROLL];
#pragma unroll
                for (int u = 0; u < DEC_UNROLL; ++u) zv[u] = i0 + 64 * u < N ? z[i0 + 64 * u] : -INFINITY;
#pragma unroll
                for (int u = 0; u < DEC_UNROLL; ++u) mx = fmaxf(mx, zv[u]);
            }
            for (int d = 32; d > 0; d >>= 1) mx = fmaxf(mx, __shfl_xor(mx, d, 64));
            float sum = 0.f;
            for (int i0 = lane; i0 < N; i0 += 64 * DEC_UNROLL) {
                float zv[DEC_UNROLL];
#pragma unroll
                for (int u = 0; u < DEC_UNROLL; ++u) zv[u] = i0 + 64 * u < N ? z[i0 + 64 * u] : 0.f;
#pragma unroll
                for (int u = 0; u < DEC_UNROLL; ++u)
                    if (i0 + 64 * u < N) sum = __fadd_rn(sum, expf(__fsub_rn(zv[u], mx)));
            }
            for (int d = 32; d > 0; d >>= 1) sum = __fadd_rn(sum, __shfl_xor(sum, d, 64));
            const bool fresh = evals == 0;                    // the first ready evaluation: q = p
            float best = -INFINITY;
            int bi = INT_MAX;
            for (int i0 = lane; i0 < N; i0 += 64 * DEC_UNROLL) {
                float zv[DEC_UNROLL], qv[DEC_UNROLL];
#pragma unroll
                for (int u = 0; u < DEC_UNROLL; ++u) {
                    const bool in = i0 + 64 * u < N;
                    zv[u] = in ? z[i0 + 64 * u] : 0.f;
                    qv[u] = in && !fresh ? qs[i0 + 64 * u] : 0.f;
                }
#pragma unroll
                for (int u = 0; u < DEC_UNROLL; ++u) {
                    const int i = i0 + 64 * u;
                    if (i >= N) break;
                    const float p = __fdiv_rn(expf(__fsub_rn(zv[u], mx)), sum);
                    const float v = fresh ? p : __fadd_rn(__fmul_rn(keep, qv[u]), __fmul_rn(alpha, p));
                    qs[i] = v;
                    if (v > best) { best = v; bi = i; }       // ascending i: the lowest index of a lane's maximum
                }
            }
            for (int d = 32; d > 0; d >>= 1) {
                const float ob = __shfl_xor(best, d, 64);
                const int oi = __shfl_xor(bi, d, 64);
                if (ob > best || (ob == best && oi < bi)) { best = ob; bi = oi; }
            }
            if (bi >= N) bi = 0;                              // no entry compares (a NaN row): class 0, conf -inf, no event
            top = bi;
            conf = best;
            if (lane == 0) {
                int run = w->run, fired = w->fired;
                if (!fresh && top == w->top) {
                    run = run < INT_MAX ? run + 1 : run;
                } else {
                    run = 1;
                    fired = 0;
                }
                if (run >= hold && conf >= thr && fired == 0 && top != blank) {
                    fired = 1;
                    emit = true;
                    w->events += 1;
                }
                w->top = top;
                w->conf = conf;
                w->run = run;
                w->fired = fired;
                w->evals = evals + 1;
            }
        }
        if (lane == 0) {
            sh_emit[s] = emit ? 1 : 0;
            sh_top[s] = top;
            sh_conf[s] = conf;
            sh_eval[s] = evals;
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {                                   // one writer of the log: stream order
        int64_t cnt = hd->log_count, ovf = hd->overflow;
        hwgat_stream_event* log = reinterpret_cast<hwgat_stream_event*>(words_of(state, S));
        bool any = false;
        for (int s = 0; s < S; ++s) {
            if (!sh_emit[s]) continue;
            any = true;
            if (cnt >= 0 && cnt < (int64_t)log_capacity) {
                hwgat_stream_event ev;
                ev.frames_seen = words_of(state, s)->frames_seen;
                ev.evaluation = sh_eval[s];
                ev.stream = s;
                ev.cls = sh_top[s];
                ev.conf = sh_conf[s];
                ev.pad = 0;
                log[cnt] = ev;
                cnt += 1;
            } else {
                ovf += 1;
            }
        }
        if (any) {
            hd->log_count = cnt;
            hd->overflow = ovf;
        }
    }
}

bool streams_ok(int n_streams) { return n_streams > 0 && n_streams <= HWGAT_STREAM_MAX_STREAMS; }
bool aligned8(const void* p) { return (((uintptr_t)p) & 7) == 0; }

}  // namespace

extern "C" int64_t hwgat_stream_state_bytes(int n_streams, int log_capacity) {
    if (!streams_ok(n_streams) || log_capacity < 0 || log_capacity > HWGAT_STREAM_MAX_LOG) return HWGAT_EINVAL;
    return (int64_t)sizeof(hwgat_stream_header) + (int64_t)n_streams * sizeof(hwgat_stream_words) +
           (int64_t)log_capacity * sizeof(hwgat_stream_event);
}

extern "C" int hwgat_stream_push(float* ring, void* state, const float* frames, const int32_t* n_new, int n_streams,
                                 int ring_frames, int push_frames, int J, int C, void* stream) {
    if (!ring || !state || !aligned8(state) || !frames || !n_new || n_streams <= 0 || ring_frames <= 0 || push_frames <= 0 ||
        J <= 0)
        return HWGAT_EINVAL;
    if (C != 2 && C != 3) return HWGAT_ESHAPE;
    if (!streams_ok(n_streams) || ring_frames > HWGAT_AUG_MAX_FRAMES || push_frames > ring_frames || J > STREAM_MAX_JOINTS)
        return HWGAT_ESHAPE;
    stream_push_k<<<n_streams, PUSH_THREADS, 0, (hipStream_t)stream>>>(ring, state, frames, n_new, ring_frames, push_frames,
                                                                        J * C);
    HWGAT_LAUNCH_CHECK();
}

extern "C" int hwgat_stream_window(const float* ring, void* state, float* clip, int32_t* clip_off, int32_t* src, double* prm,
                                   int n_streams, int ring_frames, int window_frames, int min_frames, int src_len, int J,
                                   int C, int origin, int anchor0, int anchor1, const int32_t* hands, void* stream) {
    if (!ring || !state || !aligned8(state) || !clip || !clip_off || !src || !prm || !aligned8(prm) || !hands ||
        n_streams <= 0 || ring_frames <= 0 || window_frames <= 0 || min_frames <= 0 || src_len <= 0 || J <= 0)
        return HWGAT_EINVAL;
    if (C != 2 && C != 3) return HWGAT_ESHAPE;
    if (!streams_ok(n_streams) || ring_frames > HWGAT_AUG_MAX_FRAMES || window_frames > ring_frames || J > STREAM_MAX_JOINTS ||
        src_len > (1 << 20))
        return HWGAT_ESHAPE;
    // hands = {l0, l1, lw, r0, r1, rw} (host memory), as hwgat_aug_hand_fill takes them: the origin and the anchors are
    // joints of the frame outside both hands (the hand fill rewrites hand joints; the normalisation reads the raw ring)
    const int norm[3] = {origin, anchor0, anchor1};
    for (int h = 0; h < 2; ++h) {
        const int a = hands[3 * h], e = hands[3 * h + 1];
        if (a < 0 || e <= a || e > J) return HWGAT_ESHAPE;
        for (int k = 0; k < 3; ++k)
            if (norm[k] >= a && norm[k] < e) return HWGAT_ESHAPE;
    }
    for (int k = 0; k < 3; ++k)
        if (norm[k] < 0 || norm[k] >= J) return HWGAT_ESHAPE;
    stream_window_k<<<n_streams, WIN_THREADS, 0, (hipStream_t)stream>>>(ring, state, clip, clip_off, src, prm, n_streams,
                                                                         ring_frames, window_frames, min_frames, src_len, J,
                                                                         C, origin, anchor0, anchor1);
    HWGAT_LAUNCH_CHECK();
}

extern "C" int hwgat_stream_decide(void* state, float* q, const float* logits, int n_streams, int n_classes, int log_capacity,
                                   void* stream) {
    if (!state || !aligned8(state) || !q || !logits || n_streams <= 0 || n_classes <= 0 || log_capacity < 0) return HWGAT_EINVAL;
    if (!streams_ok(n_streams) || n_classes > HWGAT_STREAM_MAX_CLASSES || log_capacity > HWGAT_STREAM_MAX_LOG) return HWGAT_ESHAPE;
    stream_decide_k<<<1, DEC_THREADS, 0, (hipStream_t)stream>>>(state, q, logits, n_streams, n_classes, log_capacity);
    HWGAT_LAUNCH_CHECK();
}
