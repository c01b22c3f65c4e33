// weight / bias gradients on 64x64 dW tiles (gemm_tn64.hip): the shapes the 128- and 256-wide tile kernels do not take
#pragma once
#include "common.h"

// N % 64 == K % 64 == 0 and N % 128 or K % 128 non-zero (stage widths that are odd multiples of 64, and their qkv / FFN)
inline bool hwgat_tn64_takes(int N, int K) { return N > 0 && K > 0 && N % 64 == 0 && K % 64 == 0 && (N % 128 || K % 128); }
// workspace of a launch with partial images: n_split x (N K + N) floats, in bytes
int64_t hwgat_tn64_ws_bytes(int64_t M, int N, int K);
// dW[N,K] += dropmask(A)[M,N]^T . ln(B)[M,K], db[N] += colsum(dropmask(A)) for A, B of `dtype`.  ws != NULL (at least
// hwgat_tn64_ws_bytes, need not be zeroed): every M split stores its partial tiles into its own image and one pass adds
// the images in split order; ws == NULL: one split per tile adds into dW / db itself.  No float atomics either way.
int hwgat_tn64_run(int dtype, const void* A, const void* B, float* dW, float* db, int64_t M, int N, int K, uint32_t pro_seed,
                   float pro_p, const float* mean, const float* rstd, const float* gamma, const float* beta,
                   const uint32_t* seed_base, float* ws, int64_t ws_bytes, hipStream_t st);
