// LayerNorm kernels for the row widths d = 64 n <= 1024 outside {128, 256, 512, 1024} (layernorm_w64.hip); the host
// dispatch of layernorm.hip routes to them.  Records as ln_args.h describes them; there is no weighted pool here.
#pragma once
#include "ln_args.h"

bool hwgat_lnw_takes(int d);
int hwgat_lnw_fwd(const void* x, const float* gm, const float* bt, void* y, float* mean, float* rstd, int64_t N, int d,
                  int dtype, hipStream_t st);
int hwgat_lnw_bwd(const LnBwdArgs& a, hipStream_t st);        // with the deterministic reductions, where a.det_ws
int hwgat_lnw_pool_fwd(const LnPoolArgs& a, hipStream_t st);  // the launch alone: lnpool_reduce_k is the caller's
int hwgat_lnw_pool_bwd(const LnPoolArgs& a, hipStream_t st);
