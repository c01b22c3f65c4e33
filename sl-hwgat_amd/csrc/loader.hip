// Device-resident clip store and train input pipeline for gfx950 (data.DeviceClipStore / data.DeviceLoader).  The input was
// the one part of a train step that waited on the host every batch: AugmentBatcher packs clips and AugRecords in a Python
// loop that scales with B, and TrainTransform.draw replays the reference's RNG calls on the CPU.  Keypoint datasets are a
// GB or two, so the whole dataset lives on the device, and two kernels make "the next batch" with every changing value in
// device words (layout, hashes and formulas: include/hwgat_hip.h, "device-resident clip store"), so that
// select -> draw -> hwgat_aug_hand_fill -> hwgat_aug_resample is one HIP graph:
//
//   loader_select_k  ONE workgroup, a thread per batch row: the row's sample index from (cursor, rank, world), the clip id
//                    through a keyed Feistel permutation of [0, n_clips) with cycle walking, the draw key, the label, the clip
//                    lengths and their prefix sums (an LDS scan), the row count; then it moves the cursor / the epoch.
//   loader_draw_k    one workgroup per row: copies the clip's raw frames into the packed batch, writes the masked bytes (a
//                    Feistel-permuted subset), the fp64 parameter record (Box-Muller normals, lanes 0..10 one each) and the
//                    composed frame map of TemporalAugmentation + TemporalSample (per-frame counts in LDS, integer atomics,
//                    one scan, a binary search per output frame).
//
// These are latency kernels (a batch is a MB or two).  No float atomics and no cross-workgroup communication: every word has
// one writer per launch.  Every index formed from a device word is reduced to its range before use.  All stores are plain
// vector stores.
#include <math.h>

#include "common.h"
#include "fused_ops.h"
#include "keyed_perm.h"
#include "linspace.h"

namespace {

static_assert(sizeof(hwgat_loader_state) == 64, "the state is 8 words");

constexpr int SEL_THREADS = HWGAT_LOADER_MAX_BATCH;           // a thread per row
constexpr int DRAW_THREADS = 256, DRAW_PER = HWGAT_AUG_MAX_FRAMES / DRAW_THREADS;
constexpr int LOADER_MAX_JOINTS = 1024, LOADER_MAX_CLIPS = 1 << 30, LOADER_MAX_WORLD = 1 << 20;
constexpr int N_NORMALS = 11;                                 // shear origin 3, shear, rotation origin 3, angles 3, shift
static_assert(DRAW_PER * DRAW_THREADS == HWGAT_AUG_MAX_FRAMES, "the scan covers every frame counter");

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }
__device__ __forceinline__ int64_t clampl(int64_t v, int64_t lo, int64_t hi) { return min(max(v, lo), hi); }

__device__ __forceinline__ double box_muller(uint32_t key, uint32_t tag, uint32_t i) {
    const double u1 = uniform01(key, tag, 2u * i), u2 = uniform01(key, tag, 2u * i + 1u);
    return __dmul_rn(sqrt(__dmul_rn(-2.0, log(u1))), cos(__dmul_rn(6.283185307179586, u2)));
}
__device__ __forceinline__ double clip01(double v) { return fmin(fmax(v, 0.0), 1.0); }

__global__ __launch_bounds__(SEL_THREADS) void loader_select_k(hwgat_loader_state* st, const int64_t* __restrict__ clip_off,
                                                               const int64_t* __restrict__ labels, int32_t* __restrict__ ids,
                                                               uint32_t* __restrict__ keys, int32_t* __restrict__ clip_len,
                                                               int32_t* __restrict__ batch_off, int64_t* __restrict__ y,
                                                               int32_t* __restrict__ n_rows, int n_clips, int64_t store_frames,
                                                               int batch, int max_frames) {
    __shared__ int sh[SEL_THREADS];
    const int r = threadIdx.x;
    const uint32_t seed = st->seed, epoch = st->epoch;
    const int nc = clampi(st->n_clips, 1, n_clips), Bd = clampi(st->batch, 1, batch);
    const int world = clampi(st->world, 1, LOADER_MAX_WORLD), rank = clampi(st->rank, 0, world - 1), flags = st->flags;
    const bool drop_last = (flags & HWGAT_LOADER_DROP_LAST) != 0;
    const int per = drop_last ? nc / world : (nc + world - 1) / world;
    const int nb0 = drop_last ? per / Bd : (per + Bd - 1) / Bd;
    const int nb = max(nb0, 1);
    const int64_t limit = drop_last ? (int64_t)nb0 * Bd * world : (int64_t)nc;       // <= nc
    int cursor = st->cursor % nb;
    if (cursor < 0) cursor += nb;
    __syncthreads();                                          // every thread has the words before thread 0 moves them
    const int64_t s = ((int64_t)cursor * Bd + r) * world + rank;
    const bool valid = r < Bd && s < limit;
    int id = -1, len = 0;
    uint32_t key = 0u;
    int64_t lab = 0;
    if (valid) {
        id = (flags & HWGAT_LOADER_SHUFFLE) ? (int)perm(mix32(seed, (uint64_t)epoch), (uint32_t)nc, (uint32_t)s) : (int)s;
        id = clampi(id, 0, nc - 1);
        const int64_t f0 = clampl(clip_off[id], 0, store_frames);
        len = (int)clampl(clip_off[id + 1] - f0, 0, min((int64_t)max_frames, store_frames - f0));
        key = mix32(mix32(seed, (1ull << 32) | (uint64_t)epoch), (uint64_t)id);
        lab = labels[id];
    }
    // inclusive prefix sums of the lengths (Hillis-Steele in LDS); the sum is at most batch * max_frames < 2^31
    sh[r] = len;
    __syncthreads();
    for (int d = 1; d < SEL_THREADS; d <<= 1) {
        const int v = r >= d ? sh[r - d] : 0;
        __syncthreads();
        sh[r] += v;
        __syncthreads();
    }
    const int rows = __syncthreads_count(valid);
    if (r < batch) {
        ids[r] = id;
        keys[r] = key;
        clip_len[r] = len;
        y[r] = lab;
        batch_off[r + 1] = sh[r];
    }
    if (r == 0) {
        batch_off[0] = 0;
        *n_rows = rows;
        if (cursor + 1 >= nb) {
            st->cursor = 0;
            st->epoch = epoch + 1u;
        } else {
            st->cursor = cursor + 1;
        }
    }
}

template <int C>
__global__ __launch_bounds__(DRAW_THREADS) void loader_draw_k(
        const hwgat_loader_state* __restrict__ st, const float* __restrict__ frames, const int64_t* __restrict__ clip_off,
        const float* __restrict__ norm, const int32_t* __restrict__ ids, const uint32_t* __restrict__ keys,
        const int32_t* __restrict__ batch_off, float* __restrict__ clip, uint8_t* __restrict__ masked,
        int32_t* __restrict__ src, double* __restrict__ prm, int n_clips, int64_t store_frames, int batch, int max_frames,
        int n, int J, double mask_p, double ratio_lo, double ratio_hi, double shear_std, double rotation_std,
        int random_sample, int random_shift) {
    __shared__ int cnt[HWGAT_AUG_MAX_FRAMES];
    __shared__ int part[DRAW_THREADS];
    __shared__ double sh_nrm[N_NORMALS + 1];
    __shared__ double sh_prm[HWGAT_AUG_NPRM];
    const int r = blockIdx.x, t = threadIdx.x, JC = J * C;
    const int id = clampi(ids[r], -1, n_clips - 1);
    const uint32_t key = keys[r];
    // the row's clip in the store and its place in the packed batch, each reduced to its buffer
    int T = 0;
    int64_t f0 = 0;
    if (id >= 0) {
        f0 = clampl(clip_off[id], 0, store_frames);
        T = (int)clampl((int64_t)batch_off[r + 1] - (int64_t)batch_off[r], 0, min((int64_t)max_frames, store_frames - f0));
    }
    const int boff = (int)clampl(batch_off[r], 0, (int64_t)batch * max_frames - T);
    const bool train = T > 0 && (st->flags & HWGAT_LOADER_TRAIN) != 0;

    // 1. the raw frames: 16-byte vectors where the source and the destination share their alignment
    {
        const float* sp = frames + f0 * JC;
        float* dp = clip + (int64_t)boff * JC;
        const int cn = T * JC;
        if ((((uintptr_t)sp ^ (uintptr_t)dp) & 15) == 0) {
            const int head = min(cn, (int)(((16 - ((uintptr_t)sp & 15)) & 15) >> 2));
            const int nv = (cn - head) >> 2;
            if (t < head) dp[t] = sp[t];
            const f32x4* sv = reinterpret_cast<const f32x4*>(sp + head);
            f32x4* dv = reinterpret_cast<f32x4*>(dp + head);
            for (int e = t; e < nv; e += DRAW_THREADS) dv[e] = sv[e];
            for (int e = head + 4 * nv + t; e < cn; e += DRAW_THREADS) dp[e] = sp[e];
        } else {
            for (int e = t; e < cn; e += DRAW_THREADS) dp[e] = sp[e];
        }
    }

    // 2. KeypointMasking: frame f is masked iff its place in a keyed permutation of [0, T) is below int(p T)
    const int n_mask = train ? clampi((int)__dmul_rn(mask_p, (double)T), 0, T) : 0;
    for (int f = t; f < T; f += DRAW_THREADS)
        masked[(int64_t)boff + f] =
            (train && perm(key + HWGAT_LOADER_TAG_MASK, (uint32_t)T, (uint32_t)f) < (uint32_t)n_mask) ? 1 : 0;

    // 3. the normals, one per lane
    if (t < N_NORMALS) {
        uint32_t tag = HWGAT_LOADER_TAG_SHIFT, idx = 0u;
        double loc = 0.5, scale = 0.1;
        if (t < 3) { tag = HWGAT_LOADER_TAG_SHEAR_ORIGIN; idx = t; }
        else if (t == 3) { tag = HWGAT_LOADER_TAG_SHEAR; loc = 0.0; scale = shear_std; }
        else if (t < 7) { tag = HWGAT_LOADER_TAG_ROT_ORIGIN; idx = t - 4; }
        else if (t < 10) { tag = HWGAT_LOADER_TAG_ROT; idx = t - 7; loc = 0.0; scale = rotation_std; }
        sh_nrm[t] = __dadd_rn(loc, __dmul_rn(scale, box_muller(key, tag, idx)));
    }
    for (int f = t; f < T; f += DRAW_THREADS) cnt[f] = 0;
    __syncthreads();

    // TemporalAugmentation's length and mode (uniform: every thread computes them)
    int L = T;
    bool random = false, subset = false;
    if (train) {
        const double ratio = __dadd_rn(__dmul_rn(__dsub_rn(ratio_hi, ratio_lo), uniform01(key, HWGAT_LOADER_TAG_RATIO, 0u)),
                                       ratio_lo);
        L = clampi((int)__dmul_rn((double)T, ratio), 1, 2 * HWGAT_AUG_MAX_FRAMES);
        random = random_sample != 0 && mix32(key + HWGAT_LOADER_TAG_MODE, 0ull) < 0x80000000u;
        subset = ratio <= 1.0;
        if (subset) L = min(L, T);
    }
    const bool pad = T > 0 && L <= n;
    int start = 0;
    if (pad) {
        const double s = (train && random_shift != 0) ? clip01(sh_nrm[10]) : 0.5;
        start = clampi((int)__dmul_rn((double)(n - L), s), 0, n - L);
    }

    // the parameter record
    if (t == 0) {
        double* p = sh_prm;
        for (int k = 0; k < HWGAT_AUG_NPRM; ++k) p[k] = 0.0;
        p[3] = 1.0;
        p[11] = p[15] = p[19] = 1.0;
        if (T > 0) {
            const float* nv = norm + (int64_t)id * 4;
            for (int c = 0; c < C; ++c) p[c] = (double)nv[c];
            p[3] = (double)nv[3];
        }
        if (train) {
            for (int c = 0; c < C; ++c) {
                p[4 + c] = clip01(sh_nrm[c]);
                p[8 + c] = clip01(sh_nrm[4 + c]);
            }
            p[7] = sh_nrm[3];
            if (C == 2) {
                const double a = sh_nrm[7], cs = cos(a), sn = sin(a);
                p[11] = cs; p[12] = -sn; p[14] = sn; p[15] = cs;
            } else {
                const double d2r = 0.017453292519943295;
                const double a0 = __dmul_rn(__dmul_rn(sh_nrm[7], 90.0), d2r), a1 = __dmul_rn(__dmul_rn(sh_nrm[8], 90.0), d2r),
                             a2 = __dmul_rn(__dmul_rn(sh_nrm[9], 90.0), d2r);
                const double c0 = cos(a0), s0 = sin(a0), c1 = cos(a1), s1 = sin(a1), c2 = cos(a2), s2 = sin(a2);
                p[11] = c2 * c1; p[12] = c2 * s1 * s0 - s2 * c0; p[13] = c2 * s1 * c0 + s2 * s0;
                p[14] = s2 * c1; p[15] = s2 * s1 * s0 + c2 * c0; p[16] = s2 * s1 * c0 - c2 * s0;
                p[17] = -s1;     p[18] = c1 * s0;                p[19] = c1 * c0;
            }
            p[20] = mix32(key + HWGAT_LOADER_TAG_FLIP, 0ull) < 0x80000000u ? 1.0 : 0.0;
        }
        p[21] = pad ? 1.0 : 0.0;
    }

    // 4. random frames: a count per frame (cnt was zeroed above), then an inclusive scan
    if (random) {
        if (subset) {
            for (int f = t; f < T; f += DRAW_THREADS)
                if (perm(key + HWGAT_LOADER_TAG_SUBSET, (uint32_t)T, (uint32_t)f) < (uint32_t)L) cnt[f] = 1;
        } else {
            for (int i = t; i < L; i += DRAW_THREADS) {
                const uint32_t h = mix32(key + HWGAT_LOADER_TAG_CHOICE, (uint64_t)i);
                const int f = (int)(((uint64_t)h * (uint64_t)T) >> 32);          // < T
                atomicAdd(&cnt[f], 1);
            }
        }
    }
    __syncthreads();
    if (random) {                                             // uniform in the workgroup
        const int base = t * DRAW_PER;
        int sum = 0;
        for (int k = 0; k < DRAW_PER; ++k)
            if (base + k < T) sum += cnt[base + k];
        part[t] = sum;
        __syncthreads();
        for (int d = 1; d < DRAW_THREADS; d <<= 1) {
            const int v = t >= d ? part[t - d] : 0;
            __syncthreads();
            part[t] += v;
            __syncthreads();
        }
        int run = part[t] - sum;
        for (int k = 0; k < DRAW_PER; ++k)
            if (base + k < T) {
                run += cnt[base + k];
                cnt[base + k] = run;
            }
        __syncthreads();
    }
    if (t < HWGAT_AUG_NPRM) prm[(int64_t)r * HWGAT_AUG_NPRM + t] = sh_prm[t];

    // the frame map: TemporalSample's entry m of the augmented clip, then that entry's raw frame
    for (int i = t; i < n; i += DRAW_THREADS) {
        int f = 0;
        if (T > 0) {
            int m;
            if (pad) m = (i >= start && i < start + L) ? i - start : (i < n / 2 ? 0 : L - 1);
            else m = linspace_int(i, L - 1, n);
            if (!train) {
                f = m;
            } else if (random) {
                int lo = 0, hi = T - 1;                       // the first frame whose cumulative count exceeds m
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    if (cnt[mid] > m) hi = mid; else lo = mid + 1;
                }
                f = lo;
            } else {
                f = linspace_int(m, T - 1, L);
            }
            f = clampi(f, 0, T - 1);
        }
        src[(int64_t)r * n + i] = f;
    }
}

bool aligned8(const void* p) { return (((uintptr_t)p) & 7) == 0; }
bool sizes_ok(int n_clips, int64_t store_frames, int batch, int max_frames) {
    return n_clips <= LOADER_MAX_CLIPS && batch <= HWGAT_LOADER_MAX_BATCH && max_frames <= HWGAT_AUG_MAX_FRAMES &&
           (int64_t)batch * max_frames < (int64_t)INT32_MAX && store_frames >= n_clips;
}

}  // namespace

extern "C" int64_t hwgat_loader_state_bytes(void) { return (int64_t)sizeof(hwgat_loader_state); }

extern "C" int hwgat_loader_select(void* state, const int64_t* clip_off, const int64_t* labels, int32_t* ids, uint32_t* keys,
                                   int32_t* clip_len, int32_t* batch_off, int64_t* y, int32_t* n_rows, int n_clips,
                                   int64_t store_frames, int batch, int max_frames, void* stream) {
    if (!state || !aligned8(state) || !clip_off || !aligned8(clip_off) || !labels || !aligned8(labels) || !ids || !keys ||
        !clip_len || !batch_off || !y || !aligned8(y) || !n_rows || n_clips <= 0 || store_frames <= 0 || batch <= 0 ||
        max_frames <= 0)
        return HWGAT_EINVAL;
    if (!sizes_ok(n_clips, store_frames, batch, max_frames)) return HWGAT_ESHAPE;
    loader_select_k<<<1, SEL_THREADS, 0, (hipStream_t)stream>>>(static_cast<hwgat_loader_state*>(state), clip_off, labels, ids,
                                                                 keys, clip_len, batch_off, y, n_rows, n_clips, store_frames,
                                                                 batch, max_frames);
    HWGAT_LAUNCH_CHECK();
}

extern "C" int hwgat_loader_draw(const void* state, const float* frames, const int64_t* clip_off, const float* norm,
                                 const int32_t* ids, const uint32_t* keys, const int32_t* batch_off, float* clip,
                                 uint8_t* masked, int32_t* src, double* prm, int n_clips, int64_t store_frames, int batch,
                                 int max_frames, int src_len, int J, int C, double mask_p, double ratio_lo, double ratio_hi,
                                 double shear_std, double rotation_std, int random_sample, int random_shift, void* stream) {
    if (!state || !aligned8(state) || !frames || !clip_off || !aligned8(clip_off) || !norm || !ids || !keys || !batch_off ||
        !clip || !masked || !src || !prm || !aligned8(prm) || n_clips <= 0 || store_frames <= 0 || batch <= 0 ||
        max_frames <= 0 || src_len <= 0 || J <= 0)
        return HWGAT_EINVAL;
    if (C != 2 && C != 3) return HWGAT_ESHAPE;
    if (!sizes_ok(n_clips, store_frames, batch, max_frames) || J > LOADER_MAX_JOINTS || src_len > (1 << 20)) return HWGAT_ESHAPE;
    // the comparisons are written so that a NaN fails them
    if (!(mask_p > 0.0 && mask_p < 1.0) || !(ratio_lo > 0.0 && ratio_lo <= ratio_hi && ratio_hi <= 2.0) ||
        !(shear_std >= 0.0 && shear_std < INFINITY) || !(rotation_std >= 0.0 && rotation_std < INFINITY))
        return HWGAT_ESHAPE;
    const hwgat_loader_state* st = static_cast<const hwgat_loader_state*>(state);
    hipStream_t hs = (hipStream_t)stream;
    if (C == 2)
        loader_draw_k<2><<<batch, DRAW_THREADS, 0, hs>>>(st, frames, clip_off, norm, ids, keys, batch_off, clip, masked, src, prm,
                                                          n_clips, store_frames, batch, max_frames, src_len, J, mask_p, ratio_lo,
                                                          ratio_hi, shear_std, rotation_std, random_sample, random_shift);
    else
        loader_draw_k<3><<<batch, DRAW_THREADS, 0, hs>>>(st, frames, clip_off, norm, ids, keys, batch_off, clip, masked, src, prm,
                                                          n_clips, store_frames, batch, max_frames, src_len, J, mask_p, ratio_lo,
                                                          ratio_hi, shear_std, rotation_std, random_sample, random_shift);
    HWGAT_LAUNCH_CHECK();
}
