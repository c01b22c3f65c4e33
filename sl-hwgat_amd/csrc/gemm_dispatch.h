// Host side of the fused linears, shared by the fp32 and the bf16 family: the table from run-time (prologue, epilogue)
// to a kernel instantiation, the validation and routing of hwgat_linear_nt_*_ex, the M split of the dW kernels and the
// deterministic dW entry.  A new prologue or epilogue is added to nt_dispatch; a new tile or dtype to a traits struct.
#pragma once
#include <type_traits>
#include "fused_ops.h"
#include "gemm_args.h"
#include "gemm_tn64.h"

template <int V> using itag = std::integral_constant<int, V>;

// Calls f(pro, epi, extra) with the compile-time tags of the kernel that runs (pro, epi): `pro` is the loader's prologue
// (PRO_LN_FOLD runs the plain loaders with the X_LNFOLD epilogue), `extra` the X_* work of the epilogue.  f launches its
// kernel and returns the status.  RELU / STAT: whether the kernel family builds the ReLU epilogues (PRO_NONE only) and
// the row-statistics epilogues (validated by the caller: PRO_NONE, EPI_BIAS_DROP_RES, whole tiles).
template <bool RELU, bool STAT, typename F>
int nt_dispatch(int pro, int epi, bool stat, bool merge, F&& f) {
    auto by_epi = [&](auto p) -> int {
        constexpr bool relu = RELU && decltype(p)::value == PRO_NONE;
        switch (epi) {
            case EPI_BIAS: return f(p, itag<EPI_BIAS>{}, itag<X_NONE>{});
            case EPI_BIAS_DROP_RES: return f(p, itag<EPI_BIAS_DROP_RES>{}, itag<X_NONE>{});
            case EPI_BIAS_GELU_DROP: return f(p, itag<EPI_BIAS_GELU_DROP>{}, itag<X_NONE>{});
            case EPI_GELU_BWD: return f(p, itag<EPI_GELU_BWD>{}, itag<X_NONE>{});
            case EPI_BIAS_GELU_DROP_G: return f(p, itag<EPI_BIAS_GELU_DROP_G>{}, itag<X_NONE>{});
            case EPI_MUL_AUX: return f(p, itag<EPI_MUL_AUX>{}, itag<X_NONE>{});
            case EPI_NONE: return f(p, itag<EPI_NONE>{}, itag<X_NONE>{});
            case EPI_BIAS_RELU_DROP:
                if constexpr (relu) return f(p, itag<EPI_BIAS_RELU_DROP>{}, itag<X_NONE>{});
                return HWGAT_EINVAL;
            case EPI_RELU_BWD:
                if constexpr (relu) return f(p, itag<EPI_RELU_BWD>{}, itag<X_NONE>{});
                return HWGAT_EINVAL;
            default: return HWGAT_EINVAL;
        }
    };
    if (stat) {
        if constexpr (STAT) {
            if (pro != PRO_NONE || epi != EPI_BIAS_DROP_RES) return HWGAT_EINVAL;
            return merge ? f(itag<PRO_NONE>{}, itag<EPI_BIAS_DROP_RES>{}, itag<X_STAT_MERGE>{})
                         : f(itag<PRO_NONE>{}, itag<EPI_BIAS_DROP_RES>{}, itag<X_STAT>{});
        }
        return HWGAT_EINVAL;
    }
    switch (pro) {
        case PRO_NONE: return by_epi(itag<PRO_NONE>{});
        case PRO_LN: return by_epi(itag<PRO_LN>{});
        case PRO_DROP: return by_epi(itag<PRO_DROP>{});
        case PRO_LN_FOLD:                                       // plain loaders, row-affine epilogue
            if (epi == EPI_BIAS) return f(itag<PRO_NONE>{}, itag<EPI_BIAS>{}, itag<X_LNFOLD>{});
            if (epi == EPI_BIAS_GELU_DROP) return f(itag<PRO_NONE>{}, itag<EPI_BIAS_GELU_DROP>{}, itag<X_LNFOLD>{});
            if (epi == EPI_BIAS_GELU_DROP_G) return f(itag<PRO_NONE>{}, itag<EPI_BIAS_GELU_DROP_G>{}, itag<X_LNFOLD>{});
            return HWGAT_EINVAL;
        default: return HWGAT_EINVAL;
    }
}

// The first m_bulk rows by `bulk`, the rest by one RAGGED launch of the 128-row tile C: loads clamp to the last row,
// stores are guarded and dropout masks are hashed with the global row index (row0), so `bulk` stays the measured code.
template <typename Tr, typename C, typename Bulk>
int nt_bulk_then_tail(const NtArgsT<typename Tr::T>& a, int64_t m_bulk, int pro, int epi, hipStream_t st, Bulk&& bulk) {
    if (m_bulk) {
        NtArgsT<typename Tr::T> b = a;
        b.M = m_bulk;
        const int rc = bulk(b);
        if (rc || m_bulk == a.M) return rc;
    }
    return Tr::template launch<C, true>(nt_rows(a, m_bulk, a.M - m_bulk), pro, epi, st);
}

// Kernel choice for a validated record.  Tr (one per dtype, next to its kernels) names the 128-row tiles Tile / Heavy /
// N64, launches them (launch<C, RAGGED>) and launches the 256-wide kernel of the dtype (launch256).
template <typename Tr>
int nt_route(const NtArgsT<typename Tr::T>& a, int pro, int epi, hipStream_t st) {
    using Args = NtArgsT<typename Tr::T>;
    using Tile = typename Tr::Tile;
    // N % 128 == 64: the 128x64 tile over the whole 128-row blocks, then a RAGGED launch for the last M % 128 rows
    // (row statistics / merged store are not built for this tile: the caller takes the separate statistics pass)
    if (a.N % 128)
        return nt_bulk_then_tail<Tr, typename Tr::N64>(a, a.M / 128 * 128, pro, epi, st, [&](const Args& b) {
            return Tr::template launch<typename Tr::N64, false>(b, pro, epi, st);
        });
    // a token count that is not a multiple of the 128-row tile: bulk launch over the aligned rows with the
    // unmodified kernels, then one small RAGGED launch for the last M % 128 rows
    if (a.M % 128)
        return nt_bulk_then_tail<Tr, Tile>(a, a.M / 128 * 128, pro, epi, st, [&](const Args& b) { return nt_route<Tr>(b, pro, epi, st); });
    // Tile choice, measured on MI355X (profiles/r01f_gemm_tile_ab.txt):
    //  - an 8-wave 256x256 tile lost to two independent 128x128 blocks per CU (110 vs 129 TF at
    //    K=512) and was removed;
    //  - four resident blocks (K16, 128 VGPRs) are 2-3 % slower than two; K slabs of 16 with THREE
    //    resident blocks per CU are ~1 % slower for plain epilogues but
    //    7-15 % faster when the epilogue is heavy (dropout+residual, GELU, GELU backward): the third
    //    block's MFMAs cover the epilogue's loads/stores.
    // (prologue-carrying launches gain nothing from K16: 570.5 vs 571.1 clips/s)
    // Outputs whose width is a multiple of 256: the 256x256 one-wave-per-SIMD kernel (gemm_f32_nt256.hip) over the
    // 256-aligned rows.  Same box, TFLOP/s, 128x128 kernels -> this one (tools/nt_lab.py, profiles/r02b_nt_lab_*.txt):
    // stage 2 plain dX 131.7 -> 143.2 and 130.4 -> 141.1, LN-prologue qkv 120.6 -> 132.1, fc1 107.8 -> 121.0, fc2 125.9 ->
    // 136.0, GELU-backward 102.7 -> 114.7, dropout-prologue dX 111.1 -> 124.3, projection 119.1 -> 126.4; stage 1 (K = 256
    // ... 768) +1 ... +10 %; stage 0 (N = 256, K = 128) +3 ... +5 %.
    // bf16: gemm_bf16_nt256.hip moves half the L2 -> LDS stream of the 128x128 tile.
    // (serving batches: fewer than 128 tiles of 256 x 256 leave most of the 256 CUs without a tile -- the 128 x 128 kernel
    //  has four times as many; B = 1 eval forward 3.96 -> see profiles/r03_serve_lab.txt)
    if (!epi_is_relu(epi) && a.N % 256 == 0 && a.K >= 128 && a.M >= 256 &&
        ((a.M / 256) * (a.N / 256) >= 128 || a.stat_sum != nullptr))     // (the row statistics of the 256-wide kernels are the order-fixed ones: eval determinism)
        // 128 rows may be left: the RAGGED instantiation hashes dropout masks with the global row index (row0)
        return nt_bulk_then_tail<Tr, Tile>(a, a.M / 256 * 256, pro, epi, st, [&](const Args& b) { return Tr::launch256(b, pro, epi, st); });
    const bool heavy = epi == EPI_BIAS_DROP_RES || epi == EPI_BIAS_GELU_DROP || epi == EPI_GELU_BWD || epi == EPI_BIAS_GELU_DROP_G || epi == EPI_MUL_AUX ||
                       epi_is_relu(epi);
    return heavy ? Tr::template launch<typename Tr::Heavy, false>(a, pro, epi, st) : Tr::template launch<Tile, false>(a, pro, epi, st);
}

// hwgat_linear_nt_*_ex: checks the arguments, builds the record and routes it.  Nothing is launched before the last check.
template <typename Tr>
int linear_nt_ex(const typename Tr::T* A, const typename Tr::T* W, const float* bias, typename Tr::T* C, int64_t M, int N, int K,
                 int pro, const float* mean, const float* rstd, const float* gamma, const float* beta, uint32_t pro_seed,
                 float pro_p, int epi, const typename Tr::T* res, typename Tr::T* C2, const typename Tr::T* aux,
                 uint32_t epi_seed, float epi_p, float* stat_sum, float* stat_sq, int merge_F, int merge_K,
                 const uint32_t* seed_base, void* stream) {
    if (!A || !W || !C || M <= 0 || N <= 0 || K <= 0) return HWGAT_EINVAL;
    if (N % 64 || K % Tr::K_GRANULE || ((M + 127) / 128) * (int64_t)(N / 64) > 0x7fffffff) return HWGAT_ESHAPE;   // any M
    if (pro == PRO_DROP && pro_p == 0.f) pro = PRO_NONE;          // eval mode: no mask to hash; checked as PRO_NONE below
    if ((pro == PRO_LN || pro == PRO_LN_FOLD) && (!mean || !rstd || !gamma || !beta)) return HWGAT_EINVAL;
    if (pro == PRO_LN_FOLD) {                                      // gamma = s[N], beta = c[N] of hwgat_ln_fold; whole tiles
        if (epi != EPI_BIAS && epi != EPI_BIAS_GELU_DROP && epi != EPI_BIAS_GELU_DROP_G) return HWGAT_EINVAL;
        if (M % 128) return HWGAT_ESHAPE;
    }
    if (epi == EPI_BIAS_DROP_RES && !res) return HWGAT_EINVAL;
    if ((epi == EPI_BIAS_GELU_DROP || epi == EPI_BIAS_GELU_DROP_G) && !C2) return HWGAT_EINVAL;
    if ((epi == EPI_GELU_BWD || epi == EPI_MUL_AUX || epi == EPI_RELU_BWD) && !aux) return HWGAT_EINVAL;
    if (pro_p < 0.f || pro_p >= 1.f || epi_p < 0.f || epi_p >= 1.f) return HWGAT_EINVAL;
    if (epi_is_relu(epi) && pro != PRO_NONE) return HWGAT_EINVAL;  // ReLU epilogues take no prologue
    if (stat_sum != nullptr || stat_sq != nullptr || merge_K > 0) { // row statistics take no prologue
        if (!stat_sum || !stat_sq || pro != PRO_NONE || epi != EPI_BIAS_DROP_RES) return HWGAT_EINVAL;
        if (M % 256) return HWGAT_ESHAPE;                          // whole tiles of either kernel only
        if (merge_K > 0 && (merge_F <= 0 || (merge_F & 1) || M % ((int64_t)merge_F * merge_K))) return HWGAT_EINVAL;
        if (N % 128) return HWGAT_ESHAPE;                          // not built for the 128x64 tile
    }
    NtArgsT<typename Tr::T> a{A, W, bias, C, C2, res, aux, mean, rstd, gamma, beta, M, N, K, pro_seed, epi_seed, pro_p, epi_p, 0,
                              stat_sum, stat_sq, merge_K > 0 ? merge_F : 0, merge_K > 0 ? merge_K : 0};
    a.seed_base = seed_base;
    return nt_route<Tr>(a, pro, epi, (hipStream_t)stream);
}

// ------------------------------------------------------------------ dW / db

// M slices per dW tile that fill `slots` resident blocks with equal blocks in whole rounds: blocks = splits x n_tiles an
// exact multiple of the slots (no nearly-empty last round), in the fewest rounds that are at least min_rounds
inline int64_t tn_round_splits(int64_t n_tiles, int64_t slots, int min_rounds) {
    auto gcd = [](int64_t x, int64_t y) { while (y) { const int64_t t = x % y; x = y; y = t; } return x; };
    const int64_t r_min = n_tiles / gcd(n_tiles, slots);
    int64_t r = r_min;
    while (r < min_rounds) r += r_min;
    return slots * r / n_tiles;
}

// The M split of a dW launch: whole rounds of equal blocks (tn_round_splits), every slice at least 16 LDS stages of
// stage_rows rows deep, rows per slice rounded up to round_to.
struct TnSplit { int n_split; int64_t rows_per_split; };
inline TnSplit tn_m_split(int64_t M, int n_tiles, int slots, int stage_rows, int round_to, int min_rounds) {
    int64_t want = tn_round_splits(n_tiles, slots, min_rounds);
    const int64_t max_split = M / (stage_rows * 16) > 0 ? M / (stage_rows * 16) : 1;
    if (want > max_split) want = max_split;
    if (want < 1) want = 1;
    int64_t rows = (M + want - 1) / want;
    rows = (rows + round_to - 1) / round_to * round_to;
    return TnSplit{(int)((M + rows - 1) / rows), rows};
}

// hwgat_linear_tn_*_det: `impl` (the dtype's tn_*_impl) stores every M split's partial dW tile / bias gradient into that
// split's image of the caller's ZERO-FILLED workspace, then one fixed-order pass adds the images: run-to-run identical
// bits.  ws_bytes >= hwgat_linear_tn_det_bytes(M, N, K); M % 32 == 0.
template <typename T, typename Impl>
int linear_tn_det(int dtype, const T* A, const T* B, float* dW, float* db, int64_t M, int N, int K, uint32_t pro_seed, float pro_p,
                  const float* mean, const float* rstd, const float* gamma, const float* beta, const uint32_t* seed_base,
                  float* ws, int64_t ws_bytes, void* stream, Impl impl) {
    if (!ws || N <= 0 || K <= 0) return HWGAT_EINVAL;
    if (hwgat_tn64_takes(N, K))
        return hwgat_tn64_run(dtype, A, B, dW, db, M, N, K, pro_seed, pro_p, mean, rstd, gamma, beta, seed_base, ws,
                              ws_bytes, (hipStream_t)stream);
    const int64_t per = (int64_t)N * K + N;
    const int64_t cap = ws_bytes / 4 / per;
    if (cap < 1) return HWGAT_ESHAPE;
    const DetWs det{ws, ws + cap * (int64_t)N * K, (int)(cap > 0x7fffffff ? 0x7fffffff : cap)};
    int rc = impl(A, B, dW, db, M, N, K, pro_seed, pro_p, mean, rstd, gamma, beta, seed_base, det, stream);
    if (rc) return rc;
    rc = hwgat_tn_det_reduce(det.dw, dW, det.cap, (int64_t)N * K, (int64_t)N * K, (hipStream_t)stream);
    if (rc || !db) return rc;
    return hwgat_tn_det_reduce(det.db, db, det.cap, N, N, (hipStream_t)stream);
}
