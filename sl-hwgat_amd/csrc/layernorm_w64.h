// LayerNorm kernels for the row widths d = 64 n <= 1024 outside {128, 256, 512, 1024} (layernorm_w64.hip); the entry
// points of layernorm.hip dispatch to them.  Arguments as the matching kernels of layernorm.hip.
#pragma once
#include "common.h"

bool hwgat_lnw_takes(int d);
int hwgat_lnw_fwd(const void* x, const float* gm, const float* bt, void* y, float* mean, float* rstd, int64_t N, int d,
                  int dtype, hipStream_t st);
// dres, dxm, xn (with bt) optional; det_ws != NULL: dgamma / dbeta through per-block images (hwgat_ln_bwd_det_bytes(d))
int hwgat_lnw_bwd(const void* dy, const void* x, const float* mean, const float* rstd, const float* gm, const float* bt,
                  const void* dres, void* dx, float* dg, float* db, int64_t N, int d, int dtype, void* dxm, uint32_t mseed,
                  float mp, void* xn, const uint32_t* sbase, float* det_ws, hipStream_t st);
int hwgat_lnw_pool_fwd(const void* x, float* xhat_sum, float* mean, float* rstd, int B, int n_tok, int chunks, int d,
                       int dtype, float* partial, hipStream_t st);
int hwgat_lnw_pool_bwd(const float* g, const void* x, const float* mean, const float* rstd, void* dx, int B, int n_tok,
                       int chunks, int d, int dtype, void* dxm, uint32_t mseed, float mp, const uint32_t* sbase,
                       hipStream_t st);
