// Input modalities for gfx950 (modality.Modality, the models' `input_modality`): the four views of a keypoint clip that the
// multi-stream skeleton recognisers train on -- joints, bones, joint motion and bone motion (formulas: include/hwgat_hip.h,
// "input modalities").  x and out are (B, T, J, C) fp32; every output entry is a copy, one IEEE subtraction, or the
// difference of two rounded subtractions, so the result is exact against any restatement in fp32.
//
//   modality_k   one thread per entry, consecutive threads on consecutive entries: row reads and stores are coalesced.  The
//                parent's coordinate lies in the same frame (J C floats, a few cache lines) and the successor's frame J C
//                floats further on, in lines the neighbouring waves fetch as their own rows; the two padding words of a
//                frame are the same address for every thread of that frame.
//
// A streaming kernel of a few megabytes: no LDS, no atomics, one pass.  The parent table is device memory, so every index
// taken from it is reduced to [0, J) before it is used.  All stores are plain vector stores.
#include "common.h"

namespace {

constexpr int MOD_THREADS = 256;

__device__ __forceinline__ float bone_of(const float* __restrict__ frame, float v, int j, int p, int C, int c) {
    return p == j ? 0.f : __fsub_rn(v, frame[p * C + c]);     // a root: +0.0 whatever the joint holds
}

__global__ __launch_bounds__(MOD_THREADS) void modality_k(const float* __restrict__ x, const int32_t* __restrict__ parent,
                                                          float* __restrict__ out, int64_t N, int T, int J, int C, int kind,
                                                          int use_pad, float pad_value) {
    const int64_t e = (int64_t)blockIdx.x * MOD_THREADS + threadIdx.x;
    if (e >= N) return;
    const float v = x[e];
    if (kind == HWGAT_MOD_JOINT) {
        out[e] = v;
        return;
    }
    const int JC = J * C;
    const int64_t f = e / JC;                                 // the frame (b, t)
    const int r = (int)(e - f * JC);
    const int t = (int)(f % T);
    const float* cur = x + f * JC;
    if (use_pad && cur[0] == pad_value) {                     // a padded frame passes through, marker and all
        out[e] = v;
        return;
    }
    const bool bones = kind == HWGAT_MOD_BONE || kind == HWGAT_MOD_BONE_MOTION;
    int j = 0, c = r, p = 0;
    if (bones) {
        j = r / C;
        c = r - j * C;
        p = min(max(parent[j], 0), J - 1);
    }
    if (kind == HWGAT_MOD_BONE) {
        out[e] = bone_of(cur, v, j, p, C, c);
        return;
    }
    const float* nxt = cur + JC;                              // read only for t < T - 1: inside the clip
    if (t == T - 1 || (use_pad && nxt[0] == pad_value)) {     // no successor to difference with
        out[e] = 0.f;
        return;
    }
    const float w = nxt[r];
    out[e] = kind == HWGAT_MOD_MOTION ? __fsub_rn(w, v)
                                      : __fsub_rn(bone_of(nxt, w, j, p, C, c), bone_of(cur, v, j, p, C, c));
}

}  // namespace

extern "C" int hwgat_modality(const float* x, const int32_t* parent, float* out, int B, int T, int J, int C, int kind,
                              int use_pad, float pad_value, void* stream) {
    if (!x || !out || B <= 0 || T <= 0 || J <= 0 || C <= 0) return HWGAT_EINVAL;
    if (kind < HWGAT_MOD_JOINT || kind > HWGAT_MOD_BONE_MOTION) return HWGAT_ESHAPE;
    if (!parent && (kind == HWGAT_MOD_BONE || kind == HWGAT_MOD_BONE_MOTION)) return HWGAT_EINVAL;
    if ((int64_t)J * C > (1 << 20)) return HWGAT_ESHAPE;      // a frame's offsets are ints
    const int64_t N = (int64_t)B * T * J * C;
    const int64_t blocks = (N + MOD_THREADS - 1) / MOD_THREADS;
    if (blocks > 0x7fffffff) return HWGAT_ESHAPE;
    if (x < out + N && out < x + N) return HWGAT_EINVAL;      // out must not overlap x: neighbours are read after stores
    modality_k<<<(unsigned)blocks, MOD_THREADS, 0, (hipStream_t)stream>>>(x, parent, out, N, T, J, C, kind, use_pad,
                                                                            pad_value);
    HWGAT_LAUNCH_CHECK();
}
