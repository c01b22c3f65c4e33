// launch records of the LayerNorm kernels (layernorm.hip, layernorm_w64.hip) and the helpers their host dispatch is
// written with.  Optional things are NULL pointers, and the kernel options follow from the record and nothing else.
#pragma once
#include "common.h"

// LayerNorm backward.  RES = dres, MASK = dx_masked (with mask_seed / mask_p / seed_base), XN = xn (with beta),
// DET = det_ws (hwgat_ln_bwd_det_bytes(d) bytes); MASK and XN exist only with RES.
struct LnBwdArgs {
    const void* dy; const void* x; const float* mean; const float* rstd; const float* gamma; const float* beta;
    const void* dres; void* dx; float* dgamma; float* dbeta;
    int64_t N; int d, dtype;
    void* dx_masked; uint32_t mask_seed; float mask_p;
    void* xn;
    const uint32_t* seed_base;
    float* det_ws;
    bool res() const { return dres != nullptr; }
    bool mask() const { return dx_masked != nullptr; }
    bool with_xn() const { return xn != nullptr; }
    bool det() const { return det_ws != nullptr; }
};

// final LayerNorm + token pool, forward (x, wtok, xhat_sum, mean, rstd, partial) and backward (the rest but xhat_sum and
// partial).  WT = wtok: the weighted pool; partial: the forward's per-block sums, added in chunk order afterwards.
struct LnPoolArgs {
    const void* x; const float* wtok; float* xhat_sum; float* mean; float* rstd;
    const float* g; void* dx; float* gdot;
    int B, n_tok, chunks, d, dtype;
    void* dx_masked; uint32_t mask_seed; float mask_p;
    const uint32_t* seed_base;
    float* partial;
    bool weighted() const { return wtok != nullptr; }
};

// ---- a run-time value as a compile-time one: f is a generic lambda, called once with a tag it reads the value from
template <typename T> struct LnElem { using type = T; };

// f(LnElem<float>) or f(LnElem<bf16_t>)
template <typename F> int ln_with_dtype(int dtype, F&& f) {
    if (dtype == HWGAT_F32) return f(LnElem<float>{});
    if (dtype == HWGAT_BF16) return f(LnElem<bf16_t>{});
    return HWGAT_EDTYPE;
}

// f(std::integral_constant<int, V>) for the V of the list that equals v; none does: HWGAT_ESHAPE
template <int... V, typename F> int ln_with_int(int v, F&& f) {
    int rc = HWGAT_ESHAPE;
    (void)((v == V && ((rc = f(std::integral_constant<int, V>{})), true)) || ...);
    return rc;
}

// f(std::true_type) or f(std::false_type)
template <typename F> int ln_with_bool(bool b, F&& f) { return b ? f(std::true_type{}) : f(std::false_type{}); }

// what follows the launch of a LayerNorm backward on `grid` blocks.  DET: the kernel wrote per-block images of 2 d floats
// into det_ws; two fixed-order reductions add them in block order onto dgamma / dbeta
inline int ln_bwd_finish(const LnBwdArgs& a, int grid, hipStream_t st) {
    if (!a.det()) HWGAT_LAUNCH_CHECK();
    const int rc = hwgat_tn_det_reduce(a.det_ws, a.dgamma, grid, 2 * (int64_t)a.d, a.d, st);
    return rc ? rc : hwgat_tn_det_reduce(a.det_ws + a.d, a.dbeta, grid, 2 * (int64_t)a.d, a.d, st);
}
