// fp32 weight-gradient GEMM with 128x128 WAVE tiles for HWGAT on gfx950: the large-output companion
// of gemm_tn_k (gemm_f32.hip), same semantics (dW += A^T B over an M slice, db += colsum(A), dropout
// mask on A, LayerNorm on B).
//
// Structure (what the vendor's best fp32 kernel does, per its disassembly -- DESIGN.md section 5):
//   * 256x256 dW tile per block, 4 waves x (128x128) = 4x4 v_mfma_f32_32x32x2_f32 tiles, the 256
//     accumulator registers live in AGPRs, ONE wave per SIMD;
//   * 16-row stages of both operands in a 3-deep LDS ring; the global loads of the stage THREE ahead are issued at
//     the top of an iteration into one of two register sets and committed to the ring in the second half of the
//     NEXT iteration (12 000 matrix-pipe cycles of lead; with one register set and 4 000 cycles the commit waited
//     on HBM: round 2); one barrier per 128 MFMAs;
//   * the steady-state loop body is branch-free straight-line code whose instruction order is PINNED
//     with sched_group_barrier: one LDS read / buffer load / LDS write (with its row's arithmetic), then 4 MFMAs,
//     repeated -- never a cluster of memory instructions with a wait, which is what idles a lone wave's MFMA pipe;
//   * every memory instruction costs the lone wave's matrix pipe cycles wherever it stands (LABLOG 10.17: ~15 per
//     ds_read2_b32, ~30 per global_load_dwordx4 with its 64-bit address arithmetic), so there are as few and as wide as
//     the data allows: a k2-step's four sub-tiles of an operand are one ds_read_b128 (a lane's sub-tiles are neighbouring
//     columns), a stage's loads are buffer loads on a scalar descriptor with loop-invariant 32-bit offsets.
#include <stdlib.h>
#include <type_traits>
#include "common.h"
#include "fused_ops.h"
#include "gemm_f32.h"
#include "gemm_dispatch.h"

namespace {

constexpr int BT = 256, TM = 16, NST = 3;
constexpr int STG = 2 * TM * BT;                                // floats per LDS stage: A[16][256] | B[16][256] = 32 KB

// LLVM SchedGroupMask bits
constexpr int SG_MFMA = 0x008, SG_VALU = 0x002, SG_VMEM_RD = 0x020, SG_DS_RD = 0x100, SG_DS_WR = 0x200;

// pin one 32-MFMA chunk: 8 groups of { one fragment read (the chunk has four: the first four groups), NVM buffer loads,
// 4 MFMAs }.  A group's memory instructions stand IN FRONT of its MFMAs (as `pin` in gemm_f32_nt256.hip): the chunk's last
// LDS read is then at least four MFMAs old when the next chunk, or the barrier, waits for it, not one instruction old.
template <int NVM = 0>
__device__ __forceinline__ void pin8() {
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        if (q < 4) __builtin_amdgcn_sched_group_barrier(SG_DS_RD, 1, 0);
        if constexpr (NVM > 0) __builtin_amdgcn_sched_group_barrier(SG_VMEM_RD, NVM, 0);
        __builtin_amdgcn_sched_group_barrier(SG_MFMA, 4, 0);
    }
}
// the committing chunk: per staged row one group for its A half (NA vector instructions, the LDS store, one fragment read,
// 4 MFMAs) and one for its B half (NB vector instructions, the LDS store, 4 MFMAs)
template <int NA, int NB>
__device__ __forceinline__ void pin_commit() {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        if constexpr (NA > 0) __builtin_amdgcn_sched_group_barrier(SG_VALU, NA, 0);
        __builtin_amdgcn_sched_group_barrier(SG_DS_WR, 1, 0);
        __builtin_amdgcn_sched_group_barrier(SG_DS_RD, 1, 0);
        __builtin_amdgcn_sched_group_barrier(SG_MFMA, 4, 0);
        if constexpr (NB > 0) __builtin_amdgcn_sched_group_barrier(SG_VALU, NB, 0);
        __builtin_amdgcn_sched_group_barrier(SG_DS_WR, 1, 0);
        __builtin_amdgcn_sched_group_barrier(SG_MFMA, 4, 0);
    }
}

#ifdef HWGAT_LAB
// lab build only: s_memtime at the start and the end of every workgroup that has an M slice, [workgroup][2], through a
// pointer set with hwgat_lab_tn256_stamps (tools/tn256_clock.py: cycles per block against the 8 192 matrix cycles of a stage)
__device__ unsigned long long* g_tn256_stamps = nullptr;
#define TN256_STAMP(i) do { if (g_tn256_stamps && threadIdx.x == 0) g_tn256_stamps[blockIdx.x * 2 + (i)] = __builtin_amdgcn_s_memtime(); } while (0)
#else
#define TN256_STAMP(i) do {} while (0)
#endif

// SLAB: the block's 256x256 partial tile goes to a workspace slab (lane-linear: every store instruction is 1 KB contiguous)
// instead of 64 MB of memory-side float atomics per launch (~49 us at the ~1.3 TB/s they sustain); tn256_reduce_k then adds
// the slabs of a tile in split order, so these weight gradients are also bit-reproducible (gemm_bf16_tn8w.hip did this first).
//   ws[(split * n_tiles + tile) * 65536 + (((wave * 16 + i * 4 + jj) * 4 + q) * 64 + lane) * 4 + e] = acc[i][jj][4 q + e]
template <int PRO, bool BLN, bool SLAB = false>
__global__ __launch_bounds__(256, 1) void gemm_tn256_k(TnArgs p, float* __restrict__ ws = nullptr) {
    HWGAT_RESOLVE_SEED1(p);
    __shared__ __attribute__((aligned(16))) float sm[NST * STG];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lq = lane & 31, hh = lane >> 5;
    const int wn = wave >> 1, wk = wave & 1;
    const int tiles_k = p.K / BT, n_tiles = (p.N / BT) * tiles_k;
    const int xcd = blockIdx.x & 7, j = blockIdx.x >> 3;
    const int tile = j % n_tiles;
    const int split = (j / n_tiles) * 8 + xcd;
    if (split >= p.n_split) return;
    const int n0 = (tile / tiles_k) * BT, k0 = (tile % tiles_k) * BT;
    const int64_t r_begin = (int64_t)split * p.rows_per_split;
    const int64_t r_end = r_begin + p.rows_per_split < p.M ? r_begin + p.rows_per_split : p.M;
    if (r_begin >= r_end) return;
    const int n_it = (int)((r_end - r_begin) / TM);
    TN256_STAMP(0);

    const int lrow = tid >> 6, lc4 = (tid & 63) * 4;            // rows lrow + 4*i (i < 4), floats lc4..lc4+3
    const uint32_t pro_th = drop_thresh(p.pro_p);
    const float pro_sc = 1.0f / (1.0f - p.pro_p);
    f32x4 ra[2][4], rb[2][4];                                   // two staging register sets (stage k uses set k & 1)
    // (mean, rstd) of a staged row in ONE register pair: the packed multiply by rstd reads its operand as a 64-bit pair, and
    // with rstd in a register of its own the pair's other half was, in one body, a statistic of the OTHER register set still
    // in flight -- the commit then waited on loads issued a chunk earlier
    f32x2 bms[2][4];
    f32x4 colsum = {0.f, 0.f, 0.f, 0.f};
    f32x4 lg = {1.f, 1.f, 1.f, 1.f}, lb = {0.f, 0.f, 0.f, 0.f};
    if constexpr (BLN) {
        lg = *reinterpret_cast<const f32x4*>(p.gamma + k0 + lc4);
        lb = *reinterpret_cast<const f32x4*>(p.beta + k0 + lc4);
    }
    // a stage's loads are BUFFER loads: a wave-uniform descriptor on the stage's first row (scalar arithmetic) + this thread's
    // 32-bit byte offsets, which never change.  Formed per thread from the row index, the 64-bit addresses were two 64-bit
    // multiplies and a chain of 64-bit adds per stage, and every global_load read a 64-bit address pair per lane (the
    // same addresses as before: the descriptor's range check is switched off by its size)
    int oa[4], ob[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) { oa[i] = ((lrow + 4 * i) * p.N + lc4) * 4; ob[i] = ((lrow + 4 * i) * p.K + lc4) * 4; }
    auto issue = [&](auto QC, int it) {
        constexpr int Q = decltype(QC)::value;
        const int64_t r0 = r_begin + (int64_t)it * TM;
        const auto da = __builtin_amdgcn_make_buffer_rsrc((void*)(p.A + r0 * p.N + n0), 0, 0x7fffffff, 0x00020000);
        const auto db = __builtin_amdgcn_make_buffer_rsrc((void*)(p.B + r0 * p.K + k0), 0, 0x7fffffff, 0x00020000);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            ra[Q][i] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(da, oa[i], 0, 0));
            rb[Q][i] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(db, ob[i], 0, 0));
            if constexpr (BLN) {
                const auto dm = __builtin_amdgcn_make_buffer_rsrc((void*)(p.mean + r0), 0, 0x7fffffff, 0x00020000);
                const auto ds = __builtin_amdgcn_make_buffer_rsrc((void*)(p.rstd + r0), 0, 0x7fffffff, 0x00020000);
                bms[Q][i].x = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(dm, (lrow + 4 * i) * 4, 0, 0));
                bms[Q][i].y = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(ds, (lrow + 4 * i) * 4, 0, 0));
            }
        }
    };
    // one staged row of a commit, in two halves (each: its counted vmcnt wait, its arithmetic, one ds_write_b128)
    auto commit_a = [&](auto QC, int so, int it, float live, int i) {
        constexpr int Q = decltype(QC)::value;
        f32x4 a = ra[Q][i];
        if constexpr (PRO == PRO_DROP) {
            const int64_t r0 = r_begin + (int64_t)it * TM + lrow;
            a *= drop_keep4(p.pro_seed, (uint64_t)(r0 + 4 * i) * p.N + n0 + lc4, pro_th, pro_sc);
        }
        colsum += a * live;
        *reinterpret_cast<f32x4*>(sm + so * STG + (lrow + 4 * i) * BT + lc4) = a;
    };
    auto commit_b = [&](auto QC, int so, int i) {
        constexpr int Q = decltype(QC)::value;
        f32x4 b = rb[Q][i];
        if constexpr (BLN) {
            f32x2 ms = bms[Q][i];
            asm("" : "+v"(ms));                                 // keeps the two in one 64-bit pair (see bms)
            b = (b - ms.x) * ms.y * lg + lb;
        }
        *reinterpret_cast<f32x4*>(sm + so * STG + TM * BT + (lrow + 4 * i) * BT + lc4) = b;
    };
    auto commit = [&](auto QC, int so, int it, float live) {
#pragma unroll
        for (int i = 0; i < 4; ++i) { commit_a(QC, so, it, live, i); commit_b(QC, so, i); }
    };

    f32x16 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int jj = 0; jj < 4; ++jj)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][jj][e] = 0.f;

    // operand chunk = 2 k2-steps (4 rows of m): 8 A + 8 B registers, each k2-step's four of an operand in ONE ds_read_b128.
    // A lane's four sub-tiles are four NEIGHBOURING columns of the staged row (sub-tile i of lane lq is n = 4 lq + i, not
    // 32 i + lq): the MFMA does not care which n a lane stands for, only the epilogue's index arithmetic does, and a
    // fragment read of 4 x 4 bytes at a stride of 128 (two ds_read2_b32) cost the lone wave's matrix pipe ~15 cycles per
    // instruction (LABLOG 10.17)
    struct Chunk { f32x4 a[2], b[2]; };
    // one quarter of a chunk's operands: j = 2 e + {0: a[e], 1: b[e]}
    auto fetch1 = [&](Chunk& c, int so, int ch, int j) {
        const int e = j >> 1;
        const int ro = (2 * (2 * ch + e) + hh) * BT + 4 * lq;
        // (assume_aligned: in one of the two bodies the compiler lost the 16 bytes of the B address and split the read)
        const float* src = sm + so * STG + ((j & 1) ? TM * BT + wk * 128 : wn * 128) + ro;
        const f32x4 v = *reinterpret_cast<const f32x4*>(__builtin_assume_aligned(src, 16));
        if (j & 1) c.b[e] = v; else c.a[e] = v;
    };
    auto fetch = [&](Chunk& c, int so, int ch) {
#pragma unroll
        for (int j = 0; j < 4; ++j) fetch1(c, so, ch, j);
    };
    auto mfma_chunk = [&](const Chunk& c) {                      // 32 MFMAs
#pragma unroll
        for (int e = 0; e < 2; ++e)
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int jj = 0; jj < 4; ++jj)
                    acc[i][jj] = __builtin_amdgcn_mfma_f32_32x32x2f32(c.a[e][i], c.b[e][jj], acc[i][jj], 0, 0, 0);
    };
    // one stage (iteration `it`, parity PAR = it & 1): 4 chunks x 32 MFMAs.
    //   the buffer loads of stage it+3 go out in chunk 0, into register set PAR^1;
    //   stage it+2 (requested a whole iteration ago, register set PAR) is written to its ring slot in chunk 2;
    //   the first operand chunk of stage it+1 is prefetched during chunk 3.
    // ONE body per parity for every stage: past the end of the M slice the loaders re-read the last stage and the
    // commit lands in a ring slot nobody reads any more (its column-sum contribution is multiplied by zero), so there
    // are no specialised tail bodies -- with ten of them the register allocator spilled 2 000+ registers.
    Chunk c0, c1;
    // vector instructions per half row of the commit, pinned in front of that half's LDS store (the model is PRO_VALU of
    // gemm_nt256_k): the column sum (and the mask hash) on A, the LayerNorm arithmetic on B
    // (the counts are what one half row compiles to, rounded up: a group that is too SMALL for its half row leaves the
    //  store behind it without its operands, and the scheduler then drops the whole chunk's pipeline -- the mask hash comes
    //  out as one lump of 200 instructions again at 46 and below, interleaved from 48 up)
    constexpr int NV_A = PRO == PRO_DROP ? 52 : 5, NV_B = BLN ? 9 : 1;
    // st, st1, st2: the ring slots of stages it, it + 1, it + 2 (rotated by the loop: no `% NST`, whose
    // strength-reduced form was a vector subtract per fragment address)
    auto stage_body = [&](auto PARC, int it, int st, int st1, int st2) {
        constexpr int PAR = decltype(PARC)::value;
        using Q = std::integral_constant<int, PAR>;
        const int it2 = it + 2 < n_it ? it + 2 : n_it - 1;
        const float live = it + 2 < n_it ? 1.0f : 0.0f;
        issue(std::integral_constant<int, PAR ^ 1>{}, it + 3 < n_it ? it + 3 : n_it - 1);
        fetch(c1, st, 1);
        mfma_chunk(c0);
        pin8<BLN ? 2 : 1>();
        __builtin_amdgcn_sched_barrier(0);
        fetch(c0, st, 2);
        mfma_chunk(c1);
        pin8<>();
        __builtin_amdgcn_sched_barrier(0);
        // (stores and reads alternate in the SOURCE too: the compiler cannot tell the two ring slots apart, so an LDS
        //  store never moves across a read that was written before it -- with the whole fetch in front of the whole
        //  commit the pinned order was unreachable and the eight stores came out as one block behind the eight reads)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            commit_a(Q{}, st2, it2, live, i);
            fetch1(c1, st, 3, i);
            commit_b(Q{}, st2, i);
        }
        mfma_chunk(c0);
        pin_commit<NV_A, NV_B>();
        __builtin_amdgcn_sched_barrier(0);
        fetch(c0, st1, 0);
        mfma_chunk(c1);
        pin8<>();
        __builtin_amdgcn_sched_barrier(0);
        __syncthreads();
    };
    using P0 = std::integral_constant<int, 0>;
    using P1 = std::integral_constant<int, 1>;

    // prologue: stages 0 and 1 into the ring, stage 2 in flight (register set 0).  n_it is even and >= 2.
    issue(P0{}, 0);
    commit(P0{}, 0, 0, 1.0f);
    issue(P1{}, 1);
    commit(P1{}, 1, 1, 1.0f);
    issue(P0{}, 2 < n_it ? 2 : n_it - 1);
    __syncthreads();
    fetch(c0, 0, 0);
#pragma nounroll
    for (int it = 0, s0 = 0, s1 = 1, s2 = 2; it < n_it; it += 2) {
        stage_body(P0{}, it, s0, s1, s2);
        stage_body(P1{}, it + 1, s1, s2, s0);
        const int t = s0; s0 = s2; s2 = s1; s1 = t;             // two stages on
    }

    const bool det = p.det_dw != nullptr;                       // deterministic mode: see TnArgs
    float* dwo = det ? p.det_dw + (int64_t)split * p.N * p.K : p.dW;
    // acc[i][jj]: lane (lq, hh), reg r -> dW[n = 4 crow(r,hh) + i][k = 4 lq + jj] of the wave's 128 x 128 (see Chunk)
    if constexpr (SLAB) {
        float* slab = ws + ((int64_t)split * n_tiles + tile) * 65536 + wave * 16384 + lane * 4;
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int jj = 0; jj < 4; ++jj)
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const f32x4 v = {acc[i][jj][4 * q], acc[i][jj][4 * q + 1], acc[i][jj][4 * q + 2], acc[i][jj][4 * q + 3]};
                    *reinterpret_cast<f32x4*>(slab + ((i * 4 + jj) * 4 + q) * 256) = v;
                }
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int jj = 0; jj < 4; ++jj)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int n = n0 + wn * 128 + 4 * crow(r, hh) + i;
                    const int k = k0 + wk * 128 + 4 * lq + jj;
                    HWGAT_TN_ACC(det, dwo, (int64_t)n * p.K + k, acc[i][jj][r]);
                }
    }
    if (p.db != nullptr && k0 == 0) {
        float* red = sm;                                        // [4][256] partial column sums
        __syncthreads();
        *reinterpret_cast<f32x4*>(red + lrow * BT + lc4) = colsum;
        __syncthreads();
        if (tid < BT) HWGAT_TN_ACC(det, det ? p.det_db + (int64_t)split * p.N : p.db, n0 + tid, red[tid] + red[BT + tid] + red[2 * BT + tid] + red[3 * BT + tid]);
    }
    TN256_STAMP(1);
}

// dW tile += the slabs of its M splits, in split order; one thread per slab float (256 workgroups per tile)
__global__ __launch_bounds__(256) void tn256_reduce_k(const float* __restrict__ ws, float* __restrict__ dW, int n_split,
                                                      int n_tiles, int tiles_k, int K) {
    const int tile = blockIdx.x >> 8;
    const int idx = (blockIdx.x & 255) * 256 + threadIdx.x;
    const float* src = ws + (int64_t)tile * 65536 + idx;
    const int64_t step = (int64_t)n_tiles * 65536;
    float s = 0.f;
    int sp = 0;
    for (; sp + 8 <= n_split; sp += 8) {                       // eight loads in flight, added in split order
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = src[(sp + j) * step];
#pragma unroll
        for (int j = 0; j < 8; ++j) s += v[j];
    }
    for (; sp < n_split; ++sp) s += src[sp * step];
    const int e = idx & 3, lane = (idx >> 2) & 63, q = (idx >> 8) & 3, t = (idx >> 10) & 15, wave = idx >> 14;
    const int i = t >> 2, jj = t & 3, lq = lane & 31, hh = lane >> 5, wn = wave >> 1, wk = wave & 1;
    const int n0 = (tile / tiles_k) * BT, k0 = (tile % tiles_k) * BT;
    dW[(int64_t)(n0 + wn * 128 + 4 * crow(4 * q + e, hh) + i) * K + k0 + wk * 128 + 4 * lq + jj] += s;
}

}  // namespace

// the M split of a launch: equal-sized blocks, one resident per CU (256 slots), whole pairs of 16-row stages
static void tn256_split(int64_t M, int n_tiles, int& n_split, int64_t& rows_per_split) {
    // The smallest whole number of rounds that fills every slot with equal blocks -- ONE round when the tile count
    // divides 256.  Every M slice ends in n_tiles x 256 KB of partial sums; the round-1 rule (at least two rounds) doubled
    // that traffic for nothing: stage 2 dWproj 112.5 -> 118.6, dW1 124.3 -> 128.0, dW2 120.0 -> 123.2 TFLOP/s on one box;
    // four rounds 104-119.  The split count has to stay a multiple of 8: split s lives on XCD s % 8 (its tiles share the
    // M slice through that XCD's L2), and 21 splits x 12 tiles put 36 blocks on five of the XCDs' 32 CUs -- twice the
    // time (measured).
    static const int min_rounds = [] { const char* e = lab_env("HWGAT_TN_ROUNDS"); return e ? atoi(e) : 1; }();
    const TnSplit sp = tn_m_split(M, n_tiles, 256, TM, 2 * TM, min_rounds);
    n_split = sp.n_split;
    rows_per_split = sp.rows_per_split;
}

// floats of workspace hwgat_launch_tn256 wants for the slab form of this shape (0: the shape does not take the kernel)
int64_t hwgat_tn256_ws_floats(int64_t M, int N, int K) {
    if (N % BT || K % BT || M % (2 * TM)) return 0;
    const int n_tiles = (N / BT) * (K / BT);
    int n_split;
    int64_t rows;
    tn256_split(M, n_tiles, n_split, rows);
    return (int64_t)n_split * n_tiles * 65536;
}

int hwgat_launch_tn256(TnArgs a, hipStream_t st, float* ws, int64_t ws_floats) {
    if (a.N % BT || a.K % BT || a.M % (2 * TM)) return HWGAT_ESHAPE;     // an even number of 16-row stages per M slice
    const int n_tiles = (a.N / BT) * (a.K / BT);
    tn256_split(a.M, n_tiles, a.n_split, a.rows_per_split);
    if (a.det_dw) {                                              // deterministic mode: plain images, never the slabs
        if (a.n_split > a.det_cap) return HWGAT_ESHAPE;
        ws = nullptr;
    }
    const int grid = ((a.n_split + 7) / 8) * 8 * n_tiles;
    const bool drop = a.pro_p > 0.f, ln = a.mean != nullptr;
    if (drop && ln) return HWGAT_ESHAPE;                         // not used by the model
    if (ws && ws_floats >= (int64_t)a.n_split * n_tiles * 65536) {
        if (drop) gemm_tn256_k<PRO_DROP, false, true><<<grid, 256, 0, st>>>(a, ws);
        else if (ln) gemm_tn256_k<PRO_NONE, true, true><<<grid, 256, 0, st>>>(a, ws);
        else gemm_tn256_k<PRO_NONE, false, true><<<grid, 256, 0, st>>>(a, ws);
        tn256_reduce_k<<<n_tiles * 256, 256, 0, st>>>(ws, a.dW, a.n_split, n_tiles, a.K / BT, a.K);
        HWGAT_LAUNCH_CHECK();
    }
    if (drop) gemm_tn256_k<PRO_DROP, false><<<grid, 256, 0, st>>>(a);
    else if (ln) gemm_tn256_k<PRO_NONE, true><<<grid, 256, 0, st>>>(a);
    else gemm_tn256_k<PRO_NONE, false><<<grid, 256, 0, st>>>(a);
    HWGAT_LAUNCH_CHECK();
}

#ifdef HWGAT_LAB
extern "C" int hwgat_lab_tn256_stamps(void* buf) {
    return hipMemcpyToSymbol(HIP_SYMBOL(g_tn256_stamps), &buf, sizeof(buf)) == hipSuccess ? 0 : HWGAT_EINVAL;
}
#endif
