// bf16 pack / unpack helpers and the launchers of the bf16 linear kernels that live in files of their own (gemm_bf16_*.hip)
#pragma once
#include "gemm_args.h"

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ void unpack8(u32x4 r, float (&v)[8]) {
    v[0] = __uint_as_float(r.x << 16); v[1] = __uint_as_float(r.x & 0xffff0000u);
    v[2] = __uint_as_float(r.y << 16); v[3] = __uint_as_float(r.y & 0xffff0000u);
    v[4] = __uint_as_float(r.z << 16); v[5] = __uint_as_float(r.z & 0xffff0000u);
    v[6] = __uint_as_float(r.w << 16); v[7] = __uint_as_float(r.w & 0xffff0000u);
}
__device__ __forceinline__ uint32_t pack2(float a, float b) {
    bf16x2 t = {(bf16_t)a, (bf16_t)b};
    return *reinterpret_cast<uint32_t*>(&t);
}
__device__ __forceinline__ u32x4 pack8(const float (&v)[8]) {
    u32x4 r = {pack2(v[0], v[1]), pack2(v[2], v[3]), pack2(v[4], v[5]), pack2(v[6], v[7])};
    return r;
}

// defined in gemm_bf16_tn256.hip: 256x256 dW tiles; N % 256 == K % 256 == M % 32 == 0
int hwgat_launch_tn256_bf16(TnArgsB a, hipStream_t st);

// defined in gemm_bf16_nt256.hip: 256x256 C tile, 4 waves x (128x128), one wave per SIMD; M % 256 == N % 256 == K % 64 == 0
int hwgat_launch_nt256_bf16(const NtArgsB& a, int pro, int epi, hipStream_t st);

// defined in gemm_bf16_tn8w.hip: 256x256 dW tiles on eight waves with LDS-DMA operand streaming; plain operands only
bool hwgat_tn8w_bf16_takes(int64_t M, int N, int K, float pro_p, const float* mean);
int hwgat_launch_tn8w_bf16(TnArgsB a, hipStream_t st, float* ws = nullptr);   // ws: hwgat_tn8w_bf16_ws_floats() floats, or NULL (atomics)
int64_t hwgat_tn8w_bf16_ws_floats(int64_t M, int N, int K);

// defined in gemm_bf16_nt8w.hip: the same tile on eight waves with LDS-DMA operand streaming and a register epilogue;
// M % 256 == N % 256 == K % 128 == 0, no A-side prologue (PRO_NONE / PRO_LN_FOLD)
bool hwgat_nt8w_bf16_takes(const NtArgsB& a, int pro, int epi);
int hwgat_launch_nt8w_bf16(const NtArgsB& a, int pro, int epi, hipStream_t st);
