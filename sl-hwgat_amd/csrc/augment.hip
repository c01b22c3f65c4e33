// Device half of the train / val-test transforms (reference hwgat/configs.py:93-108, hwgat/dataTransform.py), gfx950.
// The host (sl-hwgat_amd/augment.py) draws every random parameter of a clip; these two kernels do the array work.
//
// hand_fill: KeypointMasking's zeroing (dataTransform.py:248-252) and HandCorrection (:328-403) in place on the packed
// raw batch, one 64-lane workgroup per (clip, hand).  HandCorrection fits scipy's splrep(x, y, k=2), s = 0, once per
// missing frame, joint and coordinate; every one of those fits shares the abscissae (the hand's present frames), so
// here the collocation matrix is set up and eliminated once per (clip, hand), in fp64, with one lane per right-hand side
// (joint, coordinate).  With midpoint knots the quadratic collocation matrix is tridiagonal and totally positive, so
// elimination without pivoting is stable.  Every element is written at most once and only elements of hand frames that
// are not present are written; present frames and the wrist joints are only read, so the kernel has no
// read-after-write hazard on `x` at all.
//
// resample: NormalizeKeypoints (:84-109), ShearTransform (:131-159), RotatationTransform (:194-229), the composed
// frame map of TemporalAugmentation + TemporalSample (:264-326), RandomFlip (:111-120) and, with a gather table,
// WindowCreate (:426-455): one thread per output element, coalesced stores.
#include <algorithm>

#include "common.h"

namespace {

constexpr int AUG_ROW = 32;       // doubles per workspace row: one slot per right-hand side (hand joints x C <= 32)

// knot i of the s = 0, k = 2 spline through present frames p[0..n-1]: triple end knots, interior knots at the
// midpoints of consecutive present frames except the first and the last pair (FITPACK curfit, iopt = 0, even k)
__device__ __forceinline__ double knot(const int* p, int n, int i) {
    if (i <= 2) return (double)p[0];
    if (i >= n) return (double)p[n - 1];
    return 0.5 * ((double)p[i - 2] + (double)p[i - 1]);
}

// the three non-zero quadratic B-splines N_{l-2}, N_{l-1}, N_l at x in [t_l, t_{l+1}) (Cox-de Boor, as FITPACK fpbspl)
__device__ __forceinline__ void bspl2(const int* p, int n, int l, double x, double& n0, double& n1, double& n2) {
    const double tl = knot(p, n, l), tl1 = knot(p, n, l + 1), tlm = knot(p, n, l - 1), tl2 = knot(p, n, l + 2);
    const double left1 = x - tl, right1 = tl1 - x, left2 = x - tlm, right2 = tl2 - x;
    // degree 1
    const double a = 1.0 / (right1 + left1);
    const double d0 = right1 * a, d1 = left1 * a;
    // degree 2
    const double b0 = d0 / (right1 + left2);
    const double b1 = d1 / (right2 + left1);
    n0 = right1 * b0;
    n1 = left2 * b0 + right2 * b1;
    n2 = left1 * b1;
}

// present[f]: any coordinate of the hand's joints is non-zero in frame f and the frame is not masked
template <int C>
__device__ __forceinline__ bool hand_present(const float* clip, int f, int J, int j0, int nv, const uint8_t* msk) {
    if (msk && msk[f]) return false;
    const float* r = clip + ((int64_t)f * J + j0) * C;
    bool any = false;
    for (int e = 0; e < nv; ++e) any |= r[e] != 0.f;
    return any;
}

template <int C>
__global__ __launch_bounds__(64) void aug_hand_fill_k(float* __restrict__ x, const int32_t* __restrict__ off,
                                                      const uint8_t* __restrict__ masked, int J, int4 lhand,
                                                      int4 rhand, double* __restrict__ ws, double* __restrict__ tap,
                                                      int max_frames, int64_t total_frames) {
    extern __shared__ unsigned char aug_smem[];
    const int b = blockIdx.x >> 1, h = blockIdx.x & 1;
    const int4 hd = h ? rhand : lhand;                        // {first joint, end joint, wrist, -}
    const int j0 = hd.x, nv = (hd.y - hd.x) * C, jw = hd.z;
    const int64_t f0 = off[b];
    const int T = off[b + 1] - (int)f0;
    // the host checked both; never index LDS or the batch past them
    if (T <= 0 || T > max_frames || f0 < 0 || f0 + T > total_frames) return;
    float* clip = x + f0 * J * C;
    const uint8_t* msk = masked ? masked + f0 : nullptr;
    double* cp = reinterpret_cast<double*>(aug_smem);         // [max_frames] shared elimination factor
    int* pres = reinterpret_cast<int*>(cp + max_frames);      // [max_frames] present frames, ascending
    const int lane = threadIdx.x;

    // 1. present frames: a wave ballot per 64 frames, compacted in order into LDS
    int n = 0;
    for (int fb = 0; fb < T; fb += 64) {
        const int f = fb + lane;
        const bool pr = f < T && hand_present<C>(clip, f, J, j0, nv, msk);
        const uint64_t bal = __ballot(pr);
        if (pr) pres[n + __popcll(bal & ((1ull << lane) - 1ull))] = f;
        n += __popcll(bal);
    }
    __syncthreads();
    const int first = n ? pres[0] : T, last = n ? pres[n - 1] : -1;

    // 2. frames outside [first, last] (all frames if the hand is absent everywhere) take their frame's wrist; masked
    //    frames inside it are zero unless the spline below fills them; other absent frames are zero already.
    //    With fewer than 3 present frames splrep raises and the reference's bare `except` leaves the gaps as they are.
    const bool fit = n >= 3;
    for (int e = lane; e < T * nv; e += 64) {
        const int f = e / nv, r = e - f * nv;
        float* d = clip + ((int64_t)f * J + j0) * C + r;
        if (f < first || f > last) *d = clip[((int64_t)f * J + jw) * C + r % C];
        else if (!fit && msk && msk[f]) *d = 0.f;
    }
    if (!fit || last - first + 1 == n) return;               // nothing to interpolate

    // 3. one right-hand side per lane (lane = joint * C + coordinate); lanes >= nv carry zeros and store nothing.
    //    Forward elimination of the tridiagonal collocation system, rows j = 0..n-1 at x_j = pres[j]: row 0 and row n-1
    //    are unit rows (the triple end knots); row j in between has N_{j-1}, N_j, N_{j+1} on interval l = j + 1.
    const bool act = lane < nv;
    double* wl = ws + (2 * f0 + (int64_t)h * T) * AUG_ROW + lane;    // this lane's column, row stride AUG_ROW
    double cprev = 0.0, dprev = 0.0;
    for (int j = 0; j < n; ++j) {
        const float yv = act ? clip[((int64_t)pres[j] * J + j0) * C + lane] : 0.f;
        double a = 0.0, bb = 1.0, c = 0.0;
        if (j > 0 && j < n - 1) bspl2(pres, n, j + 1, (double)pres[j], a, bb, c);
        const double den = bb - a * cprev;
        cprev = c / den;
        dprev = ((double)yv - a * dprev) / den;
        if (lane == 0) cp[j] = cprev;
        if (act) wl[(int64_t)j * AUG_ROW] = dprev;
    }
    __syncthreads();
    // back substitution: the B-spline coefficients overwrite the lane's column
    double cnext = dprev;
    for (int j = n - 2; j >= 0; --j) {
        const double cj = act ? wl[(int64_t)j * AUG_ROW] - cp[j] * cnext : 0.0;
        if (act) wl[(int64_t)j * AUG_ROW] = cj;
        cnext = cj;
    }
    if (!act) return;
    // 4. evaluate at every absent frame in (first, last) on the knot interval t_l <= f < t_{l+1} (splev's choice)
    int k = 0, l = 2;
    for (int f = first + 1; f < last; ++f) {
        while (k < n && pres[k] < f) ++k;
        if (pres[k] == f) continue;
        const double xf = (double)f;
        while (l < n - 1 && knot(pres, n, l + 1) <= xf) ++l;
        double n0, n1, n2;
        bspl2(pres, n, l, xf, n0, n1, n2);
        const double v = n0 * wl[(int64_t)(l - 2) * AUG_ROW] + n1 * wl[(int64_t)(l - 1) * AUG_ROW]
                       + n2 * wl[(int64_t)l * AUG_ROW];
        const int64_t e = ((int64_t)f * J + j0) * C + lane;
        clip[e] = (float)v;
        if (tap) tap[f0 * J * C + e] = v;
    }
}

// per-clip parameter block (HWGAT_AUG_NPRM doubles), see include/hwgat_hip.h
template <int C>
__global__ __launch_bounds__(256) void aug_resample_k(const float* __restrict__ x, const int32_t* __restrict__ off,
                                                      const int32_t* __restrict__ src, const double* __restrict__ prm,
                                                      const int32_t* __restrict__ gather, float* __restrict__ out,
                                                      int n_out, int src_len, int J, int J_out) {
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n_out; i += gridDim.x * 256) {
        const int c = i % C;
        int r = i / C;
        const int k = r % J_out; r /= J_out;
        const int t = r % src_len;
        const int b = r / src_len;
        const int T = off[b + 1] - off[b];
        if (T <= 0) { out[i] = 0.f; continue; }                   // the host never packs an empty clip
        const int s = min(max(src[b * src_len + t], 0), T - 1);
        const int j = gather ? min(max(gather[k], 0), J - 1) : k;
        const float* xp = x + ((int64_t)off[b] + s) * J * C + (int64_t)j * C;
        const double* p = prm + (int64_t)b * HWGAT_AUG_NPRM;
        // NormalizeKeypoints in the clip's dtype (fp32), as the reference does; the quotient is formed in fp64 and
        // rounded once, which is the correctly rounded fp32 quotient (53 >= 2 * 24 + 2)
        double v[3];
#pragma unroll
        for (int q = 0; q < C; ++q) v[q] = (double)(float)((double)(xp[q] - (float)p[q]) / p[3]);
        // shear about its origin: the 2x2 [[1, s], [0, 1]] acts on the first two coordinates (row vector times matrix)
#pragma unroll
        for (int q = 0; q < C; ++q) v[q] -= p[4 + q];
        v[1] += v[0] * p[7];
#pragma unroll
        for (int q = 0; q < C; ++q) v[q] = (v[q] + p[4 + q]) - p[8 + q];     // + shear origin, - rotation origin
        // rotation about its origin: res = x @ M (M row-major 3x3 at p[11]; C = 2 uses its upper-left 2x2)
        double o = 0.0;
#pragma unroll
        for (int q = 0; q < C; ++q) o += v[q] * p[11 + q * 3 + c];
        o += p[8 + c];
        float y = (float)o;
        if (c == 0 && p[20] != 0.0) y = p[21] != 0.0 ? 1.0f - y : (float)(1.0 - o);   // RandomFlip
        out[i] = y;
    }
}

}  // namespace

extern "C" int64_t hwgat_aug_hand_fill_ws_bytes(int64_t total_frames) {
    return total_frames < 0 ? 0 : 2 * total_frames * AUG_ROW * (int64_t)sizeof(double);
}

extern "C" int hwgat_aug_hand_fill(float* x, const int32_t* clip_off, const uint8_t* masked, int n_clips,
                                   int64_t total_frames, int max_frames, int J, int C, const int32_t* hands,
                                   void* ws, int64_t ws_bytes, double* tap, void* stream) {
    if (!x || !clip_off || !hands || !ws || n_clips <= 0 || total_frames <= 0 || max_frames <= 0 || J <= 0)
        return HWGAT_EINVAL;
    if (C != 2 && C != 3) return HWGAT_ESHAPE;
    if (max_frames > HWGAT_AUG_MAX_FRAMES || n_clips > (1 << 30)) return HWGAT_ESHAPE;
    if (ws_bytes < hwgat_aug_hand_fill_ws_bytes(total_frames)) return HWGAT_EINVAL;
    // hands = {l0, l1, lw, r0, r1, rw} (host memory): two disjoint joint ranges of at most 32 / C values per frame each
    int hv[6];
    for (int i = 0; i < 6; ++i) hv[i] = hands[i];
    for (int h = 0; h < 2; ++h) {
        const int a = hv[3 * h], e = hv[3 * h + 1], w = hv[3 * h + 2];
        if (a < 0 || e <= a || e > J || (e - a) * C > AUG_ROW || w < 0 || w >= J || (w >= a && w < e))
            return HWGAT_ESHAPE;
    }
    if (hv[0] < hv[4] && hv[3] < hv[1]) return HWGAT_ESHAPE;                       // the two hands overlap
    if ((hv[2] >= hv[3] && hv[2] < hv[4]) || (hv[5] >= hv[0] && hv[5] < hv[1])) return HWGAT_ESHAPE;
    const int4 lh = make_int4(hv[0], hv[1], hv[2], 0), rh = make_int4(hv[3], hv[4], hv[5], 0);
    const size_t lds = (size_t)max_frames * (sizeof(double) + sizeof(int));
    hipStream_t st = (hipStream_t)stream;
    if (C == 2)
        aug_hand_fill_k<2><<<2 * n_clips, 64, lds, st>>>(x, clip_off, masked, J, lh, rh, (double*)ws, tap, max_frames,
                                                          total_frames);
    else
        aug_hand_fill_k<3><<<2 * n_clips, 64, lds, st>>>(x, clip_off, masked, J, lh, rh, (double*)ws, tap, max_frames,
                                                          total_frames);
    HWGAT_LAUNCH_CHECK();
}

extern "C" int hwgat_aug_resample(const float* x, const int32_t* clip_off, const int32_t* src, const double* prm,
                                  const int32_t* gather, float* out, int n_clips, int src_len, int J, int J_out, int C,
                                  void* stream) {
    if (!x || !clip_off || !src || !prm || !out || n_clips <= 0 || src_len <= 0 || J <= 0 || J_out <= 0)
        return HWGAT_EINVAL;
    if (C != 2 && C != 3) return HWGAT_ESHAPE;
    if (!gather && J_out != J) return HWGAT_ESHAPE;
    const int64_t n_out = (int64_t)n_clips * src_len * J_out * C;
    if (n_out > INT32_MAX - 8192 * 256) return HWGAT_ESHAPE;              // the grid-stride index stays in int
    const int grid = (int)std::min<int64_t>((n_out + 255) / 256, 8192);
    hipStream_t st = (hipStream_t)stream;
    if (C == 2)
        aug_resample_k<2><<<grid, 256, 0, st>>>(x, clip_off, src, prm, gather, out, (int)n_out, src_len, J, J_out);
    else
        aug_resample_k<3><<<grid, 256, 0, st>>>(x, clip_off, src, prm, gather, out, (int)n_out, src_len, J, J_out);
    HWGAT_LAUNCH_CHECK();
}
