// fp32 weight-gradient GEMM for the NARROW layers of HWGAT on gfx950 (stage 0, d = 128): the dW tile of a workgroup is
// the WHOLE weight.  Same semantics as gemm_tn_k (gemm_f32.hip): dW += A^T B over an M slice, db += colsum(A), dropout
// mask on A, LayerNorm on B.
//
// gemm_tn_k builds a 384x128 gradient as three independent 128x128 tiles, two blocks per CU, each re-reading the other
// operand; gemm_tn256_k (gemm_f32_tn256.hip) is the structure that reaches 0.91 of the sustained MFMA rate but needs
// 256-aligned shapes.  This is that structure with the tile as a template parameter:
//   * one workgroup of four waves (one per SIMD) holds all of dW in accumulators -- (N, K) = (128,128), (256,128),
//     (128,256), (384,128): at most 192 accumulator registers per lane; M is split over the 256 CUs, one slice each, so
//     every row of A and B is read from HBM once and staged in LDS once;
//   * the tile spans the full row of both operands, so a 16-row stage is ONE contiguous piece of A and one of B: the
//     loaders are flat 16-byte copies (4 KB per wave instruction), 16 x (N + K) floats per stage (<= 32 KB), 3-deep ring;
//   * two register sets of global loads (the stage three ahead is requested at the top of an iteration and committed in
//     the second half of the next one) and one straight-line body per parity whose instruction order is pinned with
//     sched_group_barrier: a few MFMAs, then LDS reads / one global load / one LDS write, repeated;
//   * the 256 partial tiles go to workspace slabs (lane-linear stores) and tnw_reduce_k adds them in split order --
//     bit-reproducible, no float atomics; without a workspace: atomics, or the split images of the deterministic mode.
#include <type_traits>
#include "common.h"
#include "fused_ops.h"
#include "gemm_f32.h"

namespace {

constexpr int TM = 16, NST = 3;

// LLVM SchedGroupMask bits
constexpr int SG_MFMA = 0x008, SG_VMEM_RD = 0x020, SG_DS_RD = 0x100, SG_DS_WR = 0x200;

// pin the instruction order of one operand chunk: 8 x { MPG MFMAs, N1 x M1, N2 x M2 }
template <int MPG, int M1, int N1, int M2, int N2>
__device__ __forceinline__ void il8() {
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        __builtin_amdgcn_sched_group_barrier(SG_MFMA, MPG, 0);
        if constexpr (N1 > 0) __builtin_amdgcn_sched_group_barrier(M1, N1, 0);
        if constexpr (N2 > 0) __builtin_amdgcn_sched_group_barrier(M2, N2, 0);
    }
}

// TN x TK = the whole weight (N == TN, K == TK); WN x (4 / WN) waves, each a (TN / WN) x (TK / WK) sub-tile of 32 x 32
// v_mfma_f32_32x32x2_f32 tiles.  Slab layout (ws != NULL), lane-linear like gemm_tn256_k's:
//   ws[split * TN * TK + ((wave * IN * JK + i * JK + jj) * 4 + q) * 256 + lane * 4 + e] = acc[i][jj][4 q + e]
template <int TN, int TK, int WN, int PRO, bool BLN>
__global__ __launch_bounds__(256, 1) void gemm_tnw_k(TnArgs p, float* __restrict__ ws) {
    HWGAT_RESOLVE_SEED1(p);
    constexpr int WK = 4 / WN, IN = TN / WN / 32, JK = TK / WK / 32;
    constexpr int NA = TN / 64, NB = TK / 64;                   // 16-byte loads per thread and stage
    constexpr int STG = TM * (TN + TK);                         // floats per LDS stage: A[16][TN] | B[16][TK]
    // a thread's i-th piece of A starts at float (tid + 256 i) * 4 of the stage: its column repeats every CP pieces
    constexpr int CP = (256 % (TN / 4)) == 0 ? 1 : 3;
    static_assert(TN % 64 == 0 && TK % 64 == 0 && (256 * CP) % (TN / 4) == 0, "tile");
    static_assert(!BLN || 256 % (TK / 4) == 0, "LayerNorm on B: one column group per thread");
    static_assert(IN * JK * 16 <= 192 && IN * WN * 32 == TN && JK * WK * 32 == TK, "sub-tile");
    __shared__ __attribute__((aligned(16))) float sm[NST * STG];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lq = lane & 31, hh = lane >> 5;
    const int wn = wave / WK, wk = wave % WK;
    const int split = blockIdx.x;
    if (split >= p.n_split) return;
    const int64_t r_begin = (int64_t)split * p.rows_per_split;
    const int64_t r_end = r_begin + p.rows_per_split < p.M ? r_begin + p.rows_per_split : p.M;
    if (r_begin >= r_end) return;
    const int n_it = (int)((r_end - r_begin) / TM);             // even and >= 2 (the launcher's split)

    const uint32_t pro_th = drop_thresh(p.pro_p);
    const float pro_sc = 1.0f / (1.0f - p.pro_p);
    f32x4 ra[2][NA], rb[2][NB];                                 // two staging register sets (stage k uses set k & 1)
    float bm[2][NB], bs[2][NB];
    f32x4 colsum[CP];
#pragma unroll
    for (int j = 0; j < CP; ++j) colsum[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    f32x4 lg = {1.f, 1.f, 1.f, 1.f}, lb = {0.f, 0.f, 0.f, 0.f};
    constexpr int BPR = TK / 4;                                 // 16-byte pieces per row of B
    if constexpr (BLN) {
        lg = *reinterpret_cast<const f32x4*>(p.gamma + (tid % BPR) * 4);
        lb = *reinterpret_cast<const f32x4*>(p.beta + (tid % BPR) * 4);
    }
    auto issue = [&](auto QC, int it) {
        constexpr int Q = decltype(QC)::value;
        const int64_t r0 = r_begin + (int64_t)it * TM;
        const float* a = p.A + r0 * TN + tid * 4;
        const float* b = p.B + r0 * TK + tid * 4;
#pragma unroll
        for (int i = 0; i < NA; ++i) ra[Q][i] = *reinterpret_cast<const f32x4*>(a + i * 1024);
#pragma unroll
        for (int i = 0; i < NB; ++i) {
            rb[Q][i] = *reinterpret_cast<const f32x4*>(b + i * 1024);
            if constexpr (BLN) {
                const int64_t row = r0 + (tid + 256 * i) / BPR;
                bm[Q][i] = p.mean[row];
                bs[Q][i] = p.rstd[row];
            }
        }
    };
    auto commit = [&](auto QC, int stage, int it, float live) {
        constexpr int Q = decltype(QC)::value;
        float* As = sm + stage * STG + tid * 4;
        float* Bs = As + TM * TN;
        const uint64_t e0 = (uint64_t)(r_begin + (int64_t)it * TM) * TN + tid * 4;   // element index of the first piece
#pragma unroll
        for (int i = 0; i < NA; ++i) {
            f32x4 a = ra[Q][i];
            if constexpr (PRO == PRO_DROP) a *= drop_keep4(p.pro_seed, e0 + i * 1024, pro_th, pro_sc);
            colsum[i % CP] += a * live;
            *reinterpret_cast<f32x4*>(As + i * 1024) = a;
        }
#pragma unroll
        for (int i = 0; i < NB; ++i) {
            f32x4 b = rb[Q][i];
            if constexpr (BLN) b = (b - bm[Q][i]) * bs[Q][i] * lg + lb;
            *reinterpret_cast<f32x4*>(Bs + i * 1024) = b;
        }
    };

    f32x16 acc[IN][JK];
#pragma unroll
    for (int i = 0; i < IN; ++i)
#pragma unroll
        for (int jj = 0; jj < JK; ++jj)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][jj][e] = 0.f;

    // operand chunk = 2 k2-steps (4 rows of m)
    struct Chunk { float a[2][IN], b[2][JK]; };
    auto fetch = [&](Chunk& c, int stage, int ch) {
        const float* As = sm + stage * STG + wn * (IN * 32) + lq;
        const float* Bs = sm + stage * STG + TM * TN + wk * (JK * 32) + lq;
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const int row = 2 * (2 * ch + e) + hh;
#pragma unroll
            for (int i = 0; i < IN; ++i) c.a[e][i] = As[row * TN + 32 * i];
#pragma unroll
            for (int jj = 0; jj < JK; ++jj) c.b[e][jj] = Bs[row * TK + 32 * jj];
        }
    };
    auto mfma_chunk = [&](const Chunk& c) {                      // 2 IN JK MFMAs
#pragma unroll
        for (int e = 0; e < 2; ++e)
#pragma unroll
            for (int i = 0; i < IN; ++i)
#pragma unroll
                for (int jj = 0; jj < JK; ++jj)
                    acc[i][jj] = __builtin_amdgcn_mfma_f32_32x32x2f32(c.a[e][i], c.b[e][jj], acc[i][jj], 0, 0, 0);
    };
    // per group of the pinned order: MFMAs, LDS reads of the next chunk, global loads (chunk 0), LDS writes (chunk 2)
    constexpr int MPG = 2 * IN * JK / 8, RPG = (2 * (IN + JK) + 7) / 8;
    constexpr int LPG = (NA + NB + (BLN ? 2 * NB : 0) + 7) / 8, WPG = (NA + NB + 7) / 8;
    static_assert(MPG * 8 == 2 * IN * JK, "MFMAs per chunk");
    // one stage (iteration `it`, parity PAR = it & 1), as in gemm_tn256_k: 4 chunks;
    //   the global loads of stage it+3 go out in chunk 0, into register set PAR^1;
    //   stage it+2 (requested a whole iteration ago, register set PAR) is written to its ring slot in chunk 2;
    //   the first operand chunk of stage it+1 is prefetched during chunk 3.
    // Past the end of the M slice the loaders re-read the last stage and the commit lands in a ring slot nobody reads
    // any more (its column-sum contribution is multiplied by zero): one body per parity, no tail bodies.
    Chunk c0, c1;
    auto stage_body = [&](auto PARC, int it) {
        constexpr int PAR = decltype(PARC)::value;
        const int st = it % NST;
        issue(std::integral_constant<int, PAR ^ 1>{}, it + 3 < n_it ? it + 3 : n_it - 1);
        fetch(c1, st, 1);
        mfma_chunk(c0);
        il8<MPG, SG_DS_RD, RPG, SG_VMEM_RD, LPG>();
        __builtin_amdgcn_sched_barrier(0);
        fetch(c0, st, 2);
        mfma_chunk(c1);
        il8<MPG, SG_DS_RD, RPG, 0, 0>();
        __builtin_amdgcn_sched_barrier(0);
        fetch(c1, st, 3);
        mfma_chunk(c0);
        commit(std::integral_constant<int, PAR>{}, (it + 2) % NST, it + 2 < n_it ? it + 2 : n_it - 1, it + 2 < n_it ? 1.0f : 0.0f);
        il8<MPG, SG_DS_RD, RPG, SG_DS_WR, WPG>();
        __builtin_amdgcn_sched_barrier(0);
        fetch(c0, (it + 1) % NST, 0);
        mfma_chunk(c1);
        il8<MPG, SG_DS_RD, RPG, 0, 0>();
        __builtin_amdgcn_sched_barrier(0);
        __syncthreads();
    };
    using P0 = std::integral_constant<int, 0>;
    using P1 = std::integral_constant<int, 1>;

    // prologue: stages 0 and 1 into the ring, stage 2 in flight (register set 0)
    issue(P0{}, 0);
    commit(P0{}, 0, 0, 1.0f);
    issue(P1{}, 1);
    commit(P1{}, 1, 1, 1.0f);
    issue(P0{}, 2 < n_it ? 2 : n_it - 1);
    __syncthreads();
    fetch(c0, 0, 0);
    for (int it = 0; it < n_it; it += 2) {
        stage_body(P0{}, it);
        stage_body(P1{}, it + 1);
    }

    const bool det = p.det_dw != nullptr;                       // deterministic mode: see TnArgs
    // D[i = n][j = k]: lane (k = lq, hh), reg r -> dW[n = crow(r,hh)][k]
    if (ws != nullptr) {
        float* slab = ws + (int64_t)split * (TN * TK) + wave * (IN * JK * 1024) + lane * 4;
#pragma unroll
        for (int i = 0; i < IN; ++i)
#pragma unroll
            for (int jj = 0; jj < JK; ++jj)
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const f32x4 v = {acc[i][jj][4 * q], acc[i][jj][4 * q + 1], acc[i][jj][4 * q + 2], acc[i][jj][4 * q + 3]};
                    *reinterpret_cast<f32x4*>(slab + ((i * JK + jj) * 4 + q) * 256) = v;
                }
    } else {
        float* dwo = det ? p.det_dw + (int64_t)split * (TN * TK) : p.dW;
#pragma unroll
        for (int i = 0; i < IN; ++i)
#pragma unroll
            for (int jj = 0; jj < JK; ++jj)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int n = wn * (IN * 32) + i * 32 + crow(r, hh);
                    const int k = wk * (JK * 32) + jj * 32 + lq;
                    HWGAT_TN_ACC(det, dwo, n * TK + k, acc[i][jj][r]);
                }
    }
    if (p.db != nullptr) {
        // partial column sums: the piece (tid + 256 j) of a stage is row (tid + 256 j) / (TN / 4) of red[SL][TN]
        constexpr int SL = 1024 * CP / TN;
        float* red = sm;                                        // the loop's last barrier is behind every LDS read
#pragma unroll
        for (int j = 0; j < CP; ++j) *reinterpret_cast<f32x4*>(red + (tid + 256 * j) * 4) = colsum[j];
        __syncthreads();
        for (int c = tid; c < TN; c += 256) {
            float s = 0.f;
#pragma unroll
            for (int q = 0; q < SL; ++q) s += red[q * TN + c];
            HWGAT_TN_ACC(det, det ? p.det_db + (int64_t)split * TN : p.db, c, s);
        }
    }
}

// dW += the slabs of the M splits, in split order; one thread per slab float
template <int TN, int TK, int WN>
__global__ __launch_bounds__(256) void tnw_reduce_k(const float* __restrict__ ws, float* __restrict__ dW, int n_split) {
    constexpr int WK = 4 / WN, IN = TN / WN / 32, JK = TK / WK / 32;
    const int idx = blockIdx.x * 256 + threadIdx.x;             // < TN * TK (the grid is exact)
    const float* src = ws + idx;
    float s = 0.f;
    int sp = 0;
    for (; sp + 8 <= n_split; sp += 8) {                       // eight loads in flight, added in split order
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = src[(int64_t)(sp + j) * (TN * TK)];
#pragma unroll
        for (int j = 0; j < 8; ++j) s += v[j];
    }
    for (; sp < n_split; ++sp) s += src[(int64_t)sp * (TN * TK)];
    const int e = idx & 3, lane = (idx >> 2) & 63, q = (idx >> 8) & 3, t = (idx >> 10) % (IN * JK), wave = idx / (IN * JK * 1024);
    const int i = t / JK, jj = t % JK, lq = lane & 31, hh = lane >> 5, wn = wave / WK, wk = wave % WK;
    dW[(wn * (IN * 32) + i * 32 + crow(4 * q + e, hh)) * TK + wk * (JK * 32) + jj * 32 + lq] += s;
}

// the M split of a launch: equal slices of whole stage pairs, at most one per CU, at least 16 stages deep
void tnw_split(int64_t M, int& n_split, int64_t& rows_per_split) {
    int64_t want = 256;
    const int64_t max_split = M / (TM * 16) > 0 ? M / (TM * 16) : 1;
    if (want > max_split) want = max_split;
    int64_t rows = (M + want - 1) / want;
    rows = (rows + 2 * TM - 1) / (2 * TM) * (2 * TM);
    n_split = (int)((M + rows - 1) / rows);
    rows_per_split = rows;
}

template <int TN, int TK, int WN>
int launch_shape(const TnArgs& a, hipStream_t st, float* ws) {
    const bool drop = a.pro_p > 0.f, ln = a.mean != nullptr;
    if (drop) gemm_tnw_k<TN, TK, WN, PRO_DROP, false><<<a.n_split, 256, 0, st>>>(a, ws);
    else if (ln) gemm_tnw_k<TN, TK, WN, PRO_NONE, true><<<a.n_split, 256, 0, st>>>(a, ws);
    else gemm_tnw_k<TN, TK, WN, PRO_NONE, false><<<a.n_split, 256, 0, st>>>(a, ws);
    if (ws) tnw_reduce_k<TN, TK, WN><<<TN * TK / 256, 256, 0, st>>>(ws, a.dW, a.n_split);
    HWGAT_LAUNCH_CHECK();
}

}  // namespace

// The launches this kernel takes: those where it beat gemm_tn_k in alternating launches on one MI355X (LABLOG 10.12).
// 128 x 128 with the dropout prologue stays on gemm_tn_k: 32 MFMAs per stage do not cover the mask hash here (-5 %).
bool hwgat_tnw_takes(int64_t M, int N, int K, float pro_p, const float* mean) {
    if (M <= 0 || M % (2 * TM) || (pro_p > 0.f && mean)) return false;      // whole stage pairs; drop + LN: not used by the model
    if (N == 128 && K == 128) return pro_p == 0.f;
    return (N == 256 && K == 128) || (N == 128 && K == 256) || (N == 384 && K == 128);
}

// floats of workspace hwgat_launch_tnw wants for the slab form of this shape (0: the shape does not take the kernel)
int64_t hwgat_tnw_ws_floats(int64_t M, int N, int K) {
    if (!hwgat_tnw_takes(M, N, K, 0.f, nullptr)) return 0;
    int n_split;
    int64_t rows;
    tnw_split(M, n_split, rows);
    return (int64_t)n_split * N * K;
}

int hwgat_launch_tnw(TnArgs a, hipStream_t st, float* ws, int64_t ws_floats) {
    if (!hwgat_tnw_takes(a.M, a.N, a.K, a.pro_p, a.mean)) return HWGAT_ESHAPE;
    tnw_split(a.M, a.n_split, a.rows_per_split);
    if (a.det_dw) {                                              // deterministic mode: plain images, never the slabs
        if (a.n_split > a.det_cap) return HWGAT_ESHAPE;
        ws = nullptr;
    }
    if (ws && ws_floats < (int64_t)a.n_split * a.N * a.K) ws = nullptr;
    if (a.N == 128 && a.K == 128) return launch_shape<128, 128, 2>(a, st, ws);
    if (a.N == 256 && a.K == 128) return launch_shape<256, 128, 2>(a, st, ws);
    if (a.N == 128 && a.K == 256) return launch_shape<128, 256, 2>(a, st, ws);
    return launch_shape<384, 128, 2>(a, st, ws);
}
