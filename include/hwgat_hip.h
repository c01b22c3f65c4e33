/*
 * hwgat_hip.h -- C ABI of libhwgat_hip.so, the MI355X (gfx950) backend for the
 * HWGAT hot path (reference: hwgat/models/HWGATE.py).
 *
 * The reference has no native interface of its own (it is 100 % Python on
 * ATen), so every entry point below cites the reference *Python* lines whose
 * arithmetic it replaces.  Conventions for all entry points:
 *
 *   - plain device pointers + sizes, no torch types; the caller owns every
 *     buffer, nothing is allocated or freed here; no global mutable state and no
 *     environment variables are read (the kernel lab's A/B switches exist only in
 *     -DHWGAT_LAB builds, csrc/common.h);
 *   - `dtype` selects activation storage: HWGAT_F32 (0) or HWGAT_BF16 (1);
 *     parameters, statistics and all arithmetic are fp32;
 *   - `stream` is a hipStream_t passed as void*; launches are asynchronous and
 *     stream-ordered; entry points are re-entrant;
 *   - return 0 on success, a negative HWGAT_E* code on bad arguments (nothing
 *     is launched then), or a positive hipError_t if the launch failed.
 *
 * Activations are kept in the natural token order (B, F, K, d) everywhere:
 * window partition / reverse / cyclic roll (HWGATE.py:30-47,197-215) are pure
 * index arithmetic inside the kernels and never materialised.
 */
#ifndef HWGAT_HIP_H
#define HWGAT_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HWGAT_F32 0
#define HWGAT_BF16 1

#define HWGAT_EINVAL (-1)   /* null pointer / non-positive size            */
#define HWGAT_ESHAPE (-2)   /* unsupported shape (head_dim, width, ...)    */
#define HWGAT_EDTYPE (-3)   /* unknown dtype code                          */

/* library / ABI version: major*1000 + minor.  The major number changes whenever an entry point is removed or its
 * argument list / code tables (pro, epi, dtype) change meaning; a binding must compare hwgat_abi_version() with the
 * HWGAT_ABI_VERSION of the header it was written against and refuse a mismatch (sl-hwgat_amd/_lib.py does).
 *   1000  round 1 (incl. hwgat_split3_bf16, hwgat_linear_nt_f32x9 -- removed in 2000)
 *   2000  round 2: *_ex linears, ln_fold / ln_finalize, epilogues 5 / 6, masked-gradient producers
 *   3000  round 3: see INTEGRATION.md section 3
 *   4000  round 4: every entry point with a dropout seed takes `const uint32_t* seed_base` in front of `stream`;
 *         hwgat_seed_set / hwgat_seed_advance; hwgat_is_lab_build; hwgat_blk_attn_*_drop, hwgat_band_attn_*_drop;
 *         hwgat_ln_bwd_det, hwgat_linear_tn_*_det (bit-reproducible parameter gradients)
 *   4001  hwgat_aug_hand_fill(_ws_bytes), hwgat_aug_resample: device-side train / eval transforms (additions only)
 *   4002  hwgat_pwin_attn_{fwd,bwd}(_drop): HWGATE part-window attention for window sizes 1..32 (additions only)
 *   4003  widths that are odd multiples of 64 (additions only): the NT linears take N % 64 == 0, the TN linears
 *         N % 64 == K % 64 == 0, the LayerNorm family every d = 64 n <= 1024
 *   4004  the Transformer baseline (additions only): hwgat_seq_attn_{fwd,bwd}, hwgat_seq_embed_{fwd,bwd}(_bytes),
 *         hwgat_seq_maxpool_{fwd,bwd}; NT epilogues 7 / 8 (ReLU + dropout and its backward)
 *         later additions under the same number (no existing signature changed): hwgat_wband_attn_{fwd,bwd}(_drop), the
 *         band attention for windows of 1..32 joints (GATE, WGATE with window_size != 16); hwgat_lnwpool_fwd(_det) /
 *         hwgat_lnwpool_bwd_masked, LayerNorm + weighted token pool (GATE)
 *   4005  the ST-GCN baseline (additions only): hwgat_stgcn_weight_prep, hwgat_stgcn_conv, hwgat_stgcn_conv_dw(_bytes),
 *         hwgat_stgcn_colsum, hwgat_stgcn_red_bytes, hwgat_stgcn_bn_{stats,eval_stats,apply,bwd},
 *         hwgat_stgcn_agg_{fwd,bwd}(_bytes), hwgat_stgcn_pool_{fwd,bwd}, hwgat_stgcn_copy_cols
 *   4006  the DecoupledGCN baseline (additions only): hwgat_dgcn_agg_{fwd,bwd}(_bytes), hwgat_dgcn_gate_{sum,apply,bwd},
 *         hwgat_dgcn_abs_sum, hwgat_dgcn_draw, hwgat_dgcn_mask_{spatial,temporal}, hwgat_dgcn_merge(_bwd),
 *         hwgat_dgcn_masked_sum
 *         later additions under the same number (additions only, no existing signature changed): hwgat_sce_{fwd,bwd}, the
 *         fused smoothed cross-entropy; hwgat_eval_accumulate, hwgat_eval_acc_bytes, the device-side evaluation accumulators;
 *         hwgat_ln_param_grads_from_g, the first block's norm1 / qkv parameter gradients without an input gradient;
 *         hwgat_optim_{set,advance,step}, Adam / AdamW over a device table with device-resident hyper-parameters;
 *         hwgat_sgd_{set,advance,step} and hwgat_nadam_{set,advance,step}, SGD and NAdam in the same form;
 *         hwgat_head_{fwd,bwd_dx,bwd_dw}, the classifier head;
 *         hwgat_gguard_{set,partial,finish,scale}, the gradient guard (global-norm clipping and non-finite detection on the
 *         device), and hwgat_gguard_{adamw,sgd,nadam}_{advance,step}, the three optimizers' launches under a guard;
 *         hwgat_bsce_{fwd,bwd}, the smoothed cross-entropy of one slice of a zero-padded batch (additions only);
 *         hwgat_wavg_{set,advance,update,swap}, EMA / equal-weight averages of the weights on the device (additions only);
 *         hwgat_meter_{bytes,fold,close}, the train meters: per-epoch sums, a step log and closed epochs kept on the
 *         device (additions only)
 *   4007  one record and one entry-point triple for the device optimizers: hwgat_opt_{set,advance,step} with a `kind` and
 *         a nullable `guard_state` replace hwgat_{optim,sgd,nadam}_{set,advance,step} and
 *         hwgat_gguard_{adamw,sgd,nadam}_{advance,step}; hwgat_opt_entry (64 bytes) is the only table record, and
 *         hwgat_gguard_{partial,scale} lose their record-size argument
 *         later additions under the same number (additions only, no existing signature changed):
 *         hwgat_stream_{state_bytes,push,window,decide}, ring-buffered keypoint streams for serve.StreamRecognizer;
 *         hwgat_loader_{state_bytes,select,draw}, the device-resident clip store's shuffle and augmentation draw for
 *         data.DeviceLoader; hwgat_attn_probs(_numel), the attention-map export of the five attention kinds;
 *         hwgat_mix_{state_bytes,set,draw,apply}, Mixup and temporal CutMix of the pairs of a batch, and
 *         hwgat_mbsce_{fwd,bwd}, the slice criterion with two targets and a weight per row;
 *         hwgat_kd_{state_bytes,set,fwd,bwd}, the same criterion distilled from a teacher's logits (additions only);
 *         hwgat_modality, the bone / motion / bone-motion views of a keypoint clip, and hwgat_ens_fuse, the fused score of
 *         an ensemble's member logits (additions only) */
#define HWGAT_ABI_VERSION 4007
int hwgat_abi_version(void);

/* ---- dropout seeds (round 4).  Every `*_seed` argument below is a SITE seed, a host integer that identifies one dropout
 * site of one block.  The seed a kernel hashes with is  site_seed + *seed_base  (32-bit wrap), where `seed_base` is a
 * DEVICE word read when the kernel runs; NULL means 0 (the site seed is then the whole seed, as before ABI 4000).
 * hwgat_seed_advance(state): state = 4 device words { step counter, base seed of the current step, initial seed, rank
 * salt }; one thread does  counter += 1; base = initial * 0x9E3779B1 + counter * 0x85EBCA77 + salt * 0x27D4EB2F.  A model
 * passes &state[1] as `seed_base` to every launch of a train step and runs hwgat_seed_advance once per step: no host
 * integer of the step depends on the step number, so the whole step can be captured in a HIP graph and replayed with
 * fresh masks (reference: nn.Dropout draws from the device generator, hwgat/models/HWGATE.py:27,116,133,135). */
int hwgat_seed_advance(uint32_t* state, void* stream);
/* the same state written from host integers (kernel arguments, no copy): state = { counter, base(counter), initial, salt }.
 * The eager path of a model calls it once per train-mode forward; after it, hwgat_seed_advance continues from `counter`. */
int hwgat_seed_set(uint32_t* state, uint32_t counter, uint32_t initial, uint32_t salt, void* stream);
/* 1 for the kernel-lab build (`python sl-hwgat_amd/build.py --lab`, libhwgat_hip_lab.so: environment switches for launch
 * parameters and instrumentation compiled in), 0 for the product library (reads no environment variables).  The lab tools assert 1 on the library they load. */
int hwgat_is_lab_build(void);

/* ---- debug: dump the lane->element maps of v_mfma_f32_32x32x2_f32 so the
 * host can verify the operand layouts the kernels assume.  out: 64*16 floats
 * = D tile of A(32x2) . B(2x32) with A[i][k] = a[i*2+k], B[k][j] = b[k*32+j]. */
int hwgat_debug_mfma32x32x2(const float* a, const float* b, float* out, void* stream);

/* ---- debug: register-only loop of `iters` x 4 x n_acc v_mfma_f32_32x32x2_f32 per wave (n_acc in
 * {4,16} independent accumulators, `blocks` x 4 waves): the attainable fp32 MFMA rate of the part. */
int hwgat_debug_mfma_peak(float* out, int blocks, int iters, int n_acc, void* stream);

/* ---- a-2/a-3/a-12: part gather + Fourier features + positional encoding.
 * Replaces WindowCreate (dataTransform.py:445-455), the Fourier mapping
 * (HWGATE.py:343-345) and PositionalEncoding's add (HWGATE.py:25-27).
 *   x    (B, T, J, C) fp32 raw keypoints
 *   idx  (K) int32 joint index per model slot, or NULL for identity (J == K)
 *   bmat (d0/2, C) fp32 frozen Gaussian matrix (state_dict key "B")
 *   pe   (T, d0) fp32 sinusoid table or NULL (pe=False)
 *   out  (B, T, K, d0) `dtype`
 *   out[..., m] = sin(p_m) + pe, out[..., d0/2+m] = cos(p_m) + pe,
 *   p_m = sum_c (2*pi*x_c) * bmat[m][c]  (fp32, accurate range reduction).
 *   drop_p > 0: PositionalEncoding's Dropout (HWGATE.py:28) applied in the same pass with the
 *   hash mask of the fused linears (element index = flat index of `out`, seed `seed`). */
int hwgat_embed_fwd(const float* x, const int32_t* idx, const float* bmat, const float* pe,
                    void* out, int B, int T, int J, int K, int C, int d0, int dtype,
                    uint32_t seed, float drop_p, const uint32_t* seed_base, void* stream);

/* ---- LayerNorm over the last axis (HWGATE.py:203, 219, 353), eps 1e-5.
 *   x, y (N, d) `dtype`; gamma, beta (d) fp32; mean, rstd (N) fp32 (saved
 *   for backward).  d in {128, 256, 512, 1024}, or (ABI 4003) any other d = 64 n <= 1024 -- 16 lanes per
 *   row, the same arithmetic; this holds for every LayerNorm entry point below (bwd, _masked, _xn, _det,
 *   lnpool).  y may be NULL: statistics only (the fused linears normalise on the fly from mean/rstd). */
int hwgat_ln_fwd(const void* x, const float* gamma, const float* beta, void* y,
                 float* mean, float* rstd, int64_t N, int d, int dtype, void* stream);

/* backward of hwgat_ln_fwd.  dx = dLN/dx (+ dres if dres != NULL, the
 * shortcut gradient of HWGATE.py:217/219); dgamma, dbeta (d) fp32 are
 * ACCUMULATED into (caller zeroes them once per step). */
int hwgat_ln_bwd(const void* dy, const void* x, const float* mean, const float* rstd,
                 const float* gamma, const void* dres, void* dx, float* dgamma, float* dbeta,
                 int64_t N, int d, int dtype, void* stream);

/* The same, plus dx_masked = dx * dropout-mask(mask_seed, element index) with keep-scale 1/(1-mask_p): the masked
 * gradient that the PRODUCER of this tensor needs in front of its Dropout (HWGATE.py:116,135 backward), written once
 * here instead of being re-hashed in the GEMM loaders that consume it.  dres is required (the block's shortcut). */
int hwgat_ln_bwd_masked(const void* dy, const void* x, const float* mean, const float* rstd,
                        const float* gamma, const void* dres, void* dx, float* dgamma, float* dbeta,
                        int64_t N, int d, int dtype, void* dx_masked, uint32_t mask_seed, float mask_p,
                        const uint32_t* seed_base, void* stream);

/* The same once more, and xn = LN(x) = xhat * gamma + beta written to `xn` (N, d) `dtype`: the layer input of the Linear
 * that follows this LayerNorm (HWGATE.py:203 -> :86, :219 -> :131), for that Linear's weight-gradient launch
 * (hwgat_linear_tn_*), which then needs no LayerNorm in its loaders.  dres required; dx_masked may be NULL. */
int hwgat_ln_bwd_xn(const void* dy, const void* x, const float* mean, const float* rstd, const float* gamma,
                    const float* beta, const void* dres, void* dx, float* dgamma, float* dbeta, int64_t N, int d,
                    int dtype, void* dx_masked, uint32_t mask_seed, float mask_p, void* xn,
                    const uint32_t* seed_base, void* stream);

/* Bit-reproducible form of the three LayerNorm-backward entry points above (round 4, "deterministic training"): every
 * option in one call -- beta and xn both given or both NULL; dres optional unless dx_masked or xn is given; dx_masked
 * optional -- and dgamma / dbeta summed in a FIXED order: each block stores its column sums into its own image of `ws`
 * (hwgat_ln_bwd_det_bytes(d) bytes, need not be zeroed) and a second pass adds the images in block order (no atomics). */
int64_t hwgat_ln_bwd_det_bytes(int d);
int hwgat_ln_bwd_det(const void* dy, const void* x, const float* mean, const float* rstd, const float* gamma,
                     const float* beta, const void* dres, void* dx, float* dgamma, float* dbeta, int64_t N, int d,
                     int dtype, void* dx_masked, uint32_t mask_seed, float mask_p, void* xn,
                     const uint32_t* seed_base, float* ws, int64_t ws_bytes, void* stream);

/* Parameter gradients of a LayerNorm -> Linear pair (y = (xhat gamma + beta) W^T + b, xhat = (x - mean) rstd) when the
 * gradient of x itself is not wanted (the first block: its input comes from the parameter-free embedding).  From
 * G[N,K] = dY^T xhat and db[N] = colsum(dY) -- one hwgat_linear_tn_* launch with gamma = 1, beta = 0 -- this ACCUMULATES
 *   dW[i][j]  += G[i][j] gamma[j] + db[i] beta[j]
 *   dgamma[j] += sum_i W[i][j] G[i][j]          dbeta[j] += sum_i db[i] W[i][j]
 * which replaces the dX GEMM and the LayerNorm-backward pass over the tokens.  All fp32; K % 32 == 0.  The sums over i run
 * in a fixed order (no atomics): the result is bit-reproducible. */
int hwgat_ln_param_grads_from_g(const float* G, const float* db, const float* W, const float* gamma, const float* beta,
                                float* dW, float* dgamma, float* dbeta, int N, int K, void* stream);

/* ---- a-4/a-5/a-6/a-10: fused window attention (MSA.forward, HWGATE.py:89-114)
 * over the body-part joint graph, with partition/roll/reverse as index math.
 *   qkv      (B, F, K, 3, nH, hd) `dtype` -- the qkv Linear output in natural
 *            token order (HWGATE.py:86 column order [q|k|v][head][hd])
 *   o        (B, F, K, nH, hd) `dtype`   -- heads concatenated (HWGATE.py:114)
 *   maskbits (2, nW, 32) uint32: bit j of word [s][w][i] = key j visible to
 *            query i in part window w; s=0 adjacency only (HWGATE.py:106-108),
 *            s=1 adjacency AND last-slot shift mask (HWGATE.py:102-104,169-187)
 *   thr      device pointer to ONE fp32 probability threshold (train mode,
 *            HWGATE.py:94-100) or NULL for eval mode
 *   shifted  1 for odd blocks (roll by -1 frame before, +1 after; HWGATE.py:197-211)
 * K = nW*16, F even, hd in {32, 64, 128}.  Semantics incl. the "== 0 -> -10000"
 * fill and uniform all-masked rows are exactly SURVEY.md 8a "MSA exact semantics". */
int hwgat_win_attn_fwd(const void* qkv, void* o, const uint32_t* maskbits, const float* thr,
                       int B, int F, int nW, int nH, int hd, int shifted, int dtype,
                       void* stream);

/* backward: do (B,F,K,nH,hd) -> dqkv (B,F,K,3,nH,hd); probabilities are
 * recomputed from qkv (+ the same thr), nothing is saved by the forward. */
int hwgat_win_attn_bwd(const void* qkv, const void* dO, void* dqkv, const uint32_t* maskbits,
                       const float* thr, int B, int F, int nW, int nH, int hd, int shifted,
                       int dtype, void* stream);

/* the same pair with ATTENTION DROPOUT (reference HWGATE.py:78,112: nn.Dropout(attn_drop) on the softmax output,
 * `attn_drop_rate` of HWGATE.py:273): the probabilities are multiplied by mask / (1 - drop_p) before the P V product.
 * The mask is a hash of (drop_seed, element index of the reference's (B f nW, nH, 32, 32) attention tensor) and is
 * recomputed by the backward: hwgat_dropout_mask_f32(out, B (F/2) nW nH 1024, drop_seed, drop_p) returns exactly it.
 * drop_p in [0, 1); drop_p > 0 needs thr (dropout exists only in train mode), else HWGAT_EINVAL.
 * hwgat_win_attn_fwd / _bwd are these with drop_p = 0. */
int hwgat_win_attn_fwd_drop(const void* qkv, void* o, const uint32_t* maskbits, const float* thr,
                            int B, int F, int nW, int nH, int hd, int shifted, int dtype,
                            uint32_t drop_seed, float drop_p, const uint32_t* seed_base, void* stream);
int hwgat_win_attn_bwd_drop(const void* qkv, const void* dO, void* dqkv, const uint32_t* maskbits,
                            const float* thr, int B, int F, int nW, int nH, int hd, int shifted,
                            int dtype, uint32_t drop_seed, float drop_p, const uint32_t* seed_base, void* stream);

/* ---- HWGATE part-window attention with a general window size W (1 <= W <= 32; W = 16 models use the entries
 * above).  A window is joints [wi W, (wi+1) W) of the frame pair (2 fi, 2 fi + 1), after the roll by one frame in
 * odd blocks (`shifted`): n = 2 W tokens, slot t = tp W + joint (HWGATE.py:30-38).  Same semantics as
 * hwgat_win_attn_*: the train-mode threshold drop over the n raw logits (thr, or NULL for eval), the adjacency and
 * shift masks, the "== 0 -> -10000" fill, the softmax over the n keys, attention dropout.
 *   qkv      (B, F, K, 3, nH, hd) `dtype`, o / dO (B, F, K, nH, hd), dqkv like qkv; K = nW W, F even, hd in {32, 64}
 *   maskbits (2, nW, n) uint64: bit j of word [s][w][i] = key slot j visible to query slot i of part window w;
 *            s=0 adjacency only, s=1 adjacency AND the last-slot same-frame mask (the last frame pair of a shifted
 *            block, HWGATE.py:169-187).  Bits >= n are ignored.
 * Attention dropout hashes the element index of the reference's (B f nW, nH, n, n) attention tensor:
 * hwgat_dropout_mask_f32(out, B (F/2) nW nH n^2, drop_seed, drop_p) is the mask.  drop_p > 0 needs thr.
 * No atomics: forward and backward are bit-reproducible.  HWGAT_ESHAPE for W outside 1..32, K % W != 0, odd F,
 * hd not in {32, 64}. */
int hwgat_pwin_attn_fwd(const void* qkv, void* o, const uint64_t* maskbits, const float* thr, int B, int F, int K,
                        int W, int nH, int hd, int shifted, int dtype, void* stream);
int hwgat_pwin_attn_bwd(const void* qkv, const void* dO, void* dqkv, const uint64_t* maskbits, const float* thr,
                        int B, int F, int K, int W, int nH, int hd, int shifted, int dtype, void* stream);
int hwgat_pwin_attn_fwd_drop(const void* qkv, void* o, const uint64_t* maskbits, const float* thr, int B, int F,
                             int K, int W, int nH, int hd, int shifted, int dtype, uint32_t drop_seed, float drop_p,
                             const uint32_t* seed_base, void* stream);
int hwgat_pwin_attn_bwd_drop(const void* qkv, const void* dO, void* dqkv, const uint64_t* maskbits, const float* thr,
                             int B, int F, int K, int W, int nH, int hd, int shifted, int dtype, uint32_t drop_seed,
                             float drop_p, const uint32_t* seed_base, void* stream);

/* ---- (f) rank 3, sibling model HGATE: fused BLOCK attention (MSA.forward of
 * hwgat/models/HGATE.py:84-108) with block_partition / block_reverse / torch.roll
 * (HGATE.py:30-47,184-207) as index math.  A block is 2 frames x KJ joints (all joints
 * of the skeleton: 29 in HGATEParams), no part windows and no train-mode threshold.
 *   qkv      (B, F, KJ, 3, nH, hd) `dtype`, o (B, F, KJ, nH, hd) `dtype`
 *   maskbits (2, 64, 2) uint32: query slot i = tp*32 + joint (tp = frame of the pair);
 *            bit j of word [s][i][kt] = key joint j of frame kt visible to query i;
 *            s=0 adjacency only (HGATE.py:100-102), s=1 adjacency AND the shift mask
 *            of the LAST block of a shifted layer (HGATE.py:96-98,154-172).  Slots
 *            with joint >= KJ are padding: never read, written or counted as keys.
 *   shifted  1 for odd blocks (roll by -1 frame before, +1 after; HGATE.py:185-207)
 * F even, 1 <= KJ <= 32, hd in {32, 64}. */
int hwgat_blk_attn_fwd(const void* qkv, void* o, const uint32_t* maskbits,
                       int B, int F, int KJ, int nH, int hd, int shifted, int dtype,
                       void* stream);

/* backward: do (B,F,KJ,nH,hd) -> dqkv (B,F,KJ,3,nH,hd); probabilities recomputed. */
int hwgat_blk_attn_bwd(const void* qkv, const void* dO, void* dqkv, const uint32_t* maskbits,
                       int B, int F, int KJ, int nH, int hd, int shifted, int dtype,
                       void* stream);

/* The same with attention dropout (reference HGATE.py:78,106: nn.Dropout on the softmax output, train mode): the
 * probabilities are multiplied by mask / (1 - drop_p), mask = the common hash over the element index of the reference's
 * (B F/2, nH, 2 KJ, 2 KJ) attention tensor (token = frame * KJ + joint): hwgat_dropout_mask_f32(out, B (F/2) nH (2 KJ)^2,
 * drop_seed, drop_p) returns exactly it.  The backward recomputes the mask.  drop_p = 0: the plain kernels, bit for bit. */
int hwgat_blk_attn_fwd_drop(const void* qkv, void* o, const uint32_t* maskbits, int B, int F, int KJ, int nH, int hd,
                            int shifted, int dtype, uint32_t drop_seed, float drop_p, const uint32_t* seed_base,
                            void* stream);
int hwgat_blk_attn_bwd_drop(const void* qkv, const void* dO, void* dqkv, const uint32_t* maskbits, int B, int F, int KJ,
                            int nH, int hd, int shifted, int dtype, uint32_t drop_seed, float drop_p,
                            const uint32_t* seed_base, void* stream);

/* ---- (f) rank 3, sibling model WGATE: fused BAND attention (MSA.forward of
 * hwgat/models/WGATE.py:87-108) with window_partition / window_reverse (WGATE.py:32-65)
 * as index math.  A WGATE window is one 16-joint part window over ALL F frames with an
 * additive 0 / -10000 mask (WGATE.py:97-100,190) from a block-tridiagonal adjacency
 * (model_params.py:209-228): only keys of frames f-1, f, f+1 can carry weight.
 *   qkv      (B, F, K, 3, nH, hd) `dtype`, o (B, F, K, nH, hd) `dtype`, K = nW*16
 *   maskrows (nW, 16) uint64: bit (16*t + j) of row [w][i] = key joint j of frame
 *            f-1+t (t = 0,1,2) visible to query joint i of frame f, the same for every f
 *            (frames outside the clip are dropped by the kernel); every row must have at
 *            least one visible key in t = 1 (the reference's adjacency has a unit diagonal)
 * hd in {16, 32}; any F >= 1. */
int hwgat_band_attn_fwd(const void* qkv, void* o, const uint64_t* maskrows,
                        int B, int F, int nW, int nH, int hd, int dtype, void* stream);

/* backward: do (B,F,K,nH,hd) -> dqkv (B,F,K,3,nH,hd); probabilities recomputed. */
int hwgat_band_attn_bwd(const void* qkv, const void* dO, void* dqkv, const uint64_t* maskrows,
                        int B, int F, int nW, int nH, int hd, int dtype, void* stream);

/* The same with attention dropout (reference WGATE.py:81,103): mask over the element index of the reference's DENSE
 * (B nW, nH, F 16, F 16) attention tensor (token = frame * 16 + joint) -- only the band entries are ever evaluated.
 * hwgat_dropout_mask_f32(out, B nW nH (F 16)^2, drop_seed, drop_p) is the whole mask. */
int hwgat_band_attn_fwd_drop(const void* qkv, void* o, const uint64_t* maskrows, int B, int F, int nW, int nH, int hd,
                             int dtype, uint32_t drop_seed, float drop_p, const uint32_t* seed_base, void* stream);
int hwgat_band_attn_bwd_drop(const void* qkv, const void* dO, void* dqkv, const uint64_t* maskrows, int B, int F, int nW,
                             int nH, int hd, int dtype, uint32_t drop_seed, float drop_p, const uint32_t* seed_base,
                             void* stream);

/* ---- wide band attention: the same band form for windows ("frames") of W <= 32 joints -- GATE (GATE.py:40-70, one
 * window = all K <= 32 joints, nW = 1) and WGATE with window_size != 16.  K = nW * W joints per frame.
 *   qkv (B,F,K,3,nH,hd), o / do (B,F,K,nH,hd), dqkv as qkv, all `dtype`
 *   maskrows (nW, 32, 3) uint32: word [w][i][t] bit j = key joint j of frame f-1+t visible to query joint i of frame f,
 *            the same for every f; rows i >= W and bits j >= W are 0.  The diagonal need not be set; a row without any
 *            visible key yields zeros.  functional.wband_mask_rows builds and validates them.
 *   1 <= W <= 32, hd in {16, 32}, any F >= 1.  fp32 storage runs fp32 MFMA, bf16 storage bf16 MFMA (softmax in fp32).
 * Results do not depend on the batch order or on how the launcher cuts a clip into frame segments, bit for bit. */
int hwgat_wband_attn_fwd(const void* qkv, void* o, const uint32_t* maskrows, int B, int F, int nW, int W, int nH, int hd,
                         int dtype, void* stream);
int hwgat_wband_attn_bwd(const void* qkv, const void* dO, void* dqkv, const uint32_t* maskrows, int B, int F, int nW,
                         int W, int nH, int hd, int dtype, void* stream);
/* ... with attention dropout: mask over the element index of the reference's DENSE (B nW, nH, F W, F W) attention tensor
 * (token = frame * W + joint); hwgat_dropout_mask_f32(out, B nW nH (F W)^2, drop_seed, drop_p) is the whole mask. */
int hwgat_wband_attn_fwd_drop(const void* qkv, void* o, const uint32_t* maskrows, int B, int F, int nW, int W, int nH,
                              int hd, int dtype, uint32_t drop_seed, float drop_p, const uint32_t* seed_base,
                              void* stream);
int hwgat_wband_attn_bwd_drop(const void* qkv, const void* dO, void* dqkv, const uint32_t* maskrows, int B, int F, int nW,
                              int W, int nH, int hd, int dtype, uint32_t drop_seed, float drop_p,
                              const uint32_t* seed_base, void* stream);

/* ---- attention-map export: the eval-mode probabilities the five fused forwards above multiply into V (no train-mode
 * threshold, no attention dropout), written out instead of kept in registers, and / or their head-mean column sums.  An
 * addition under ABI 4007 (no existing signature changed).
 *   kind     one of HWGAT_ATTN_*; qkv (B, F, K, 3, nH, hd) `dtype` and `mask` are exactly what that kind's _fwd reads
 *            (W = 16 for WIN / BAND, W = K for BLK); `shifted` as in the forward, ignored by the band kinds
 *   probs    fp32, hwgat_attn_probs_numel(...) elements, or NULL.
 *            pair kinds (WIN, PWIN, BLK): (B, F/2, nW, nH, n, n), n = 2 W, token = tp W + joint -- the reference's
 *            (B f nW, nH, n, n) attention tensor element for element (the tensor the _drop entry points index); BLK has
 *            nW = 1 and no pad slots.  In a shifted block window fi holds frames (2 fi + 1) % F and (2 fi + 2) % F.
 *            band kinds (BAND, WBAND): (B, nW, nH, F, W, 3, W); [b][w][h][f][i][t][j] = the weight query joint i of frame f
 *            gives key joint j of frame f - 1 + t; key frames outside the clip and masked entries are 0 (the whole of the
 *            reference's dense (F W)^2 row outside the band is 0 in fp32), a WBAND row without a visible key is zeros.
 *   received fp32 (B, F, K), or NULL: received[b][f][s] = (1 / nH) sum_h sum_q P_h[q -> key (f, s)], in the frame and slot
 *            coordinates of the block's INPUT (the roll of a shifted block undone).  Computed without materialising P.
 * probs and received must not both be NULL (HWGAT_EINVAL).  fp32 arithmetic for both storage dtypes.  No atomics: two runs
 * are bit-equal and a clip's values do not depend on the batch around it.  HWGAT_ESHAPE for an unknown kind and for every
 * shape the kind's _fwd refuses (hd: WIN 32 / 64 / 128, PWIN and BLK 32 / 64, BAND and WBAND 16 / 32; odd F for a pair
 * kind; W outside 1..32; K % W != 0); the shape arguments are checked before any pointer is looked at. */
#define HWGAT_ATTN_WIN 0   /* HWGATE, W = 16            mask (2,nW,32) u32   */
#define HWGAT_ATTN_PWIN 1  /* HWGATE, any W <= 32       mask (2,nW,2W) u64   */
#define HWGAT_ATTN_BLK 2   /* HGATE, W = KJ = K <= 32   mask (2,64,2) u32    */
#define HWGAT_ATTN_BAND 3  /* WGATE, W = 16             mask (nW,16) u64     */
#define HWGAT_ATTN_WBAND 4 /* GATE / WGATE W <= 32      mask (nW,32,3) u32   */
int64_t hwgat_attn_probs_numel(int kind, int B, int F, int K, int W, int nH);
int hwgat_attn_probs(int kind, const void* qkv, const void* mask, float* probs, float* received, int B, int F, int K,
                     int W, int nH, int hd, int shifted, int dtype, void* stream);

/* debug: one v_mfma_f32_16x16x4_f32 with a (16x4), b (4x16) row-major -> out (64 lanes x 4 regs) */
int hwgat_debug_mfma16x16x4(const float* a, const float* b, float* out, void* stream);

/* ---- a-11: final LayerNorm + mean over all f*K tokens (HWGATE.py:353-354).
 *   x (B, n_tok, d) `dtype`; feat (B, d) fp32 must be ZERO on entry (sums of
 *   normalised values are accumulated, then hwgat_lnpool_finish scales them);
 *   mean, rstd (B*n_tok) fp32 saved. */
int hwgat_lnpool_fwd(const void* x, float* xhat_sum, float* mean, float* rstd,
                     int B, int n_tok, int d, int dtype, void* stream);
/* Bit-reproducible form (the reference's eval() forward is deterministic, HWGATE.py:352-360): every block of the
 * launch stores its partial sum into `partial` (B * hwgat_lnpool_partial_rows(B, n_tok) * d floats, caller-owned) and a
 * second launch adds a clip's rows in index order into xhat_sum (which need NOT be zero on entry).  partial == NULL
 * is hwgat_lnpool_fwd (fp32 atomics, summation order varies from run to run). */
int hwgat_lnpool_partial_rows(int B, int n_tok);
int hwgat_lnpool_fwd_det(const void* x, float* xhat_sum, float* mean, float* rstd,
                         int B, int n_tok, int d, int dtype, float* partial, void* stream);
/* backward: g (B, d) fp32 = dfeat * gamma / n_tok  ->  dx (B, n_tok, d) */
int hwgat_lnpool_bwd(const float* g, const void* x, const float* mean, const float* rstd,
                     void* dx, int B, int n_tok, int d, int dtype, void* stream);
/* ... and dx_masked = dx * dropout-mask(mask_seed, element index), see hwgat_ln_bwd_masked (dx_masked may be NULL) */
int hwgat_lnpool_bwd_masked(const float* g, const void* x, const float* mean, const float* rstd,
                            void* dx, int B, int n_tok, int d, int dtype, void* dx_masked, uint32_t mask_seed,
                            float mask_p, const uint32_t* seed_base, void* stream);

/* ---- final LayerNorm + WEIGHTED token pool (GATE.py:181, 208-210: weightedAvg = nn.Linear(T K, 1) over the token axis):
 *   xhat_wsum[b][c] = sum_t wtok[t] xhat[b][t][c]   (the caller applies gamma, beta sum(wtok) and the bias)
 *   x (B, n_tok, d) `dtype`; wtok (n_tok) fp32; mean, rstd (B*n_tok) fp32 saved; d in {128, 256, 512, 1024}.
 *   hwgat_lnwpool_fwd: fp32 atomics, xhat_wsum must be ZERO on entry.  _det: `partial` as hwgat_lnpool_fwd_det
 *   (B * hwgat_lnpool_partial_rows(B, n_tok) * d floats), fixed summation order; partial == NULL is the atomic form. */
int hwgat_lnwpool_fwd(const void* x, const float* wtok, float* xhat_wsum, float* mean, float* rstd,
                      int B, int n_tok, int d, int dtype, void* stream);
int hwgat_lnwpool_fwd_det(const void* x, const float* wtok, float* xhat_wsum, float* mean, float* rstd,
                          int B, int n_tok, int d, int dtype, float* partial, void* stream);
/* backward: g (B, d) fp32 = dfeat * gamma -> dx (B, n_tok, d) (token t's upstream gradient is wtok[t] g[b]) and
 * gdot (B, n_tok) fp32 = sum_c g[b][c] xhat[b][t][c], the per-clip share of d wtok[t]; dx_masked / mask_* as
 * hwgat_lnpool_bwd_masked (dx_masked may be NULL). */
int hwgat_lnwpool_bwd_masked(const float* g, const float* wtok, const void* x, const float* mean, const float* rstd,
                             void* dx, float* gdot, int B, int n_tok, int d, int dtype, void* dx_masked,
                             uint32_t mask_seed, float mask_p, const uint32_t* seed_base, void* stream);

/* ---- a-9: TemporalMerging (HWGATE.py:55-63): (B,F,K,d) -> (B,F/2,K,2d),
 * out[b,fi,k,tp*d+c] = in[b,2fi+tp,k,c]; `inverse` = 1 maps gradients back. */
int hwgat_merge(const void* in, void* out, int B, int F, int K, int d, int inverse,
                int dtype, void* stream);
/* inverse mapping of a gradient plus a second, dropout-masked copy (mask of (mask_seed, un-merged element index)):
 * what the last block of a stage needs in front of its fc2 Dropout (HWGATE.py:135 backward) */
int hwgat_unmerge_masked(const void* in, void* out, void* out_masked, int B, int F, int K, int d, int dtype,
                         uint32_t mask_seed, float mask_p, const uint32_t* seed_base, void* stream);

/* ---- a-6/a-7/a-8: fp32 Linear layers on f32 MFMA with fused elementwise work.
 * Replaces nn.Linear (HWGATE.py:86,115,131,134) + bias + GELU (:132) + Dropout
 * (:116,:133,:135) + residual adds (:217,:219) forward, and their dX backward.
 *   C[M,N] = pro(A)[M,K] . W[N,K]^T, all fp32 row-major; N % 64 == K % 32 == 0, any M >= 1
 *   (a ragged last 128-row block clamps its loads to row M-1 and guards its stores).  N % 128 == 64 (ABI 4003) runs
 *   on 128x64 tiles, every pro / epi code; the _ex statistics / merged store are not built for it (HWGAT_ESHAPE).
 *   pro: 0 none | 1 LayerNorm: (A-mean[m])*rstd[m]*gamma[k]+beta[k] | 2 dropout mask on A
 *        (keep-scale 1/(1-pro_p), element index m*K+k, seed pro_seed)
 *        (pro 2 with pro_p == 0 is pro 0, fp32 and bf16 alike: it is rewritten BEFORE the arguments are checked, so
 *        an eval-mode call may carry it where a rule below says "pro 0 only")
 *        | 3 folded LayerNorm (hwgat_ln_fold below): A is the un-normalised input, W = W o gamma, gamma = s[N],
 *        beta = c[N], bias ignored; the epilogue forms rstd[m] (acc - mean[m] s[n]) + c[n] -- the value of pro 1 up
 *        to rounding, with the per-element normalisation out of the load path; epi 0 or 2 only, M % 128 == 0
 *   epi: 0  C = acc + bias
 *        1  C = res + dropout(acc + bias)             (mask index m*N+n, seed epi_seed)
 *        2  C2 = acc + bias ; C = dropout(gelu(C2))   (exact-erf GELU)
 *        3  C = acc * dropmask * gelu'(aux)           (backward of epi 2; aux = saved C2)
 *        4  C = acc
 *        5  C2 = gelu'(acc + bias) * dropmask ; C = dropout(gelu(acc + bias))   (training form of epi 2: the factor the
 *           backward needs is stored instead of the pre-activation)
 *        6  C = acc * aux                             (backward of epi 5; aux = its saved C2)
 *        7  C = dropout(relu(acc + bias))             (ABI 4004; pro 0 only)
 *        8  C = acc * (aux > 0) / (1 - epi_p)         (backward of epi 7; aux = its output C, epi_p = its p; pro 0 only)
 *   bias may be NULL (treated as 0).  For dX pass W = transposed weight. */
int hwgat_linear_nt_f32(const float* A, const float* W, const float* bias, float* C, int64_t M, int N,
                        int K, int pro, const float* mean, const float* rstd, const float* gamma,
                        const float* beta, uint32_t pro_seed, float pro_p, int epi, const float* res,
                        float* C2, const float* aux, uint32_t epi_seed, float epi_p,
                        const uint32_t* seed_base, void* stream);

/* The same launch for the two linears whose OUTPUT is the input of a LayerNorm (proj -> norm2, HWGATE.py:217-219;
 * fc2 -> the next block's norm1, :219 -> :203, through TemporalMerging :55-63 at a stage end).  Requires pro = 0,
 * epi = 1, M % 256 == 0.  In addition to hwgat_linear_nt_f32:
 *   stat_sum, stat_sq  (rows of the output) fp32, ZEROED by the caller: per-row sum / sum of squares of the stored
 *                      output values are accumulated into them (hwgat_ln_finalize then yields mean / rstd), which
 *                      removes the separate statistics pass over the tensor;
 *   merge_K > 0        the output is stored in the TemporalMerging layout: row (b, f, k) of the (B, merge_F, merge_K, N)
 *                      result goes to row (b, f/2, k), columns (f & 1) N .. (f & 1) N + N - 1 of a (B, merge_F/2,
 *                      merge_K, 2N) tensor C; statistics are then per merged row (2N values).  res stays in the
 *                      natural layout. */
int hwgat_linear_nt_f32_ex(const float* A, const float* W, const float* bias, float* C, int64_t M, int N,
                           int K, int pro, const float* mean, const float* rstd, const float* gamma,
                           const float* beta, uint32_t pro_seed, float pro_p, int epi, const float* res,
                           float* C2, const float* aux, uint32_t epi_seed, float epi_p, float* stat_sum,
                           float* stat_sq, int merge_F, int merge_K, const uint32_t* seed_base, void* stream);

/* Weights of a Linear that follows a LayerNorm (norm1 -> qkv, HWGATE.py:203-205 / :86; norm2 -> fc1, :219 / :131),
 * folded for pro = 3 of the NT launches:  Wf[n,k] = W[n,k] gamma[k] in `dtype` (HWGAT_F32 / HWGAT_BF16),
 * s[n] = sum_k Wf[n,k] (of the stored values), c[n] = bias[n] + sum_k beta[k] W[n,k].  W, bias, gamma, beta fp32
 * (the master weights); bias may be NULL.  One launch per step and linear (N x K elements). */
int hwgat_ln_fold(const float* W, const float* bias, const float* gamma, const float* beta, int N, int K,
                  void* Wf, float* s, float* c, int dtype, void* stream);

/* (row sum, row sum of squares) of a d-wide tensor -> (mean, rstd) in place, nn.LayerNorm's biased variance and
 * eps 1e-5 (HWGATE.py:162,166). */
int hwgat_ln_finalize(float* sum_mean, float* sq_rstd, int64_t n, int d, void* stream);

/* weight/bias gradient: dW[N,K] += dropmask(A)[M,N]^T . ln(B)[M,K] ; db[N] += colsum(dropmask(A))
 * (db may be NULL).  Accumulates with fp32 atomics across M slices: caller provides zeroed
 * (or to-be-accumulated-into) dW/db.  N % 128 == K % 128 == 0, any M >= 1.  pro_p == 0: no mask.
 * mean != NULL: B is LayerNorm-ed on the fly, (B-mean[m])*rstd[m]*gamma[k]+beta[k].
 * ABI 4003: N % 64 == K % 64 == 0 with N % 128 or K % 128 non-zero runs on 64x64 dW tiles WITHOUT float atomics, in both
 * dtypes and every prologue: with a workspace (the _ws / _det entry points; hwgat_linear_tn_{f32,bf16}_ws_bytes and
 * hwgat_linear_tn_det_bytes return its size, it need not be zeroed) each M split stores its partial tile and one pass
 * adds the partials in split order -- bit-reproducible, any M; without one (these plain entry points) one block per
 * tile walks all of M, which is correct but slow for large M. */
int hwgat_linear_tn_f32(const float* A, const float* B, float* dW, float* db, int64_t M, int N, int K,
                        uint32_t pro_seed, float pro_p, const float* mean, const float* rstd,
                        const float* gamma, const float* beta, const uint32_t* seed_base, void* stream);

/* ---- BASELINE config 3: the same two linears with bf16 activations / weights on
 * v_mfma_f32_32x32x16_bf16 (fp32 accumulate).  A, W, C, C2, res, aux are bf16; bias, LN
 * statistics/affine, dW, db stay fp32.  Semantics, prologue/epilogue codes and dropout masks are
 * identical to the fp32 entry points (any M >= 1: a ragged tail gets its own small launch); K % 64 == 0 here, and the same
 * N % 64 / 64x64 dW-tile rules (ABI 4003) as the fp32 entry points. */
int hwgat_linear_nt_bf16(const void* A, const void* W, const float* bias, void* C, int64_t M, int N, int K,
                         int pro, const float* mean, const float* rstd, const float* gamma,
                         const float* beta, uint32_t pro_seed, float pro_p, int epi, const void* res,
                         void* C2, const void* aux, uint32_t epi_seed, float epi_p,
                         const uint32_t* seed_base, void* stream);
/* hwgat_linear_nt_f32_ex for bf16 activations: the statistics are those of the bf16-rounded output values (what the
 * next LayerNorm reads), the merged store writes bf16. */
int hwgat_linear_nt_bf16_ex(const void* A, const void* W, const float* bias, void* C, int64_t M, int N, int K,
                            int pro, const float* mean, const float* rstd, const float* gamma,
                            const float* beta, uint32_t pro_seed, float pro_p, int epi, const void* res,
                            void* C2, const void* aux, uint32_t epi_seed, float epi_p, float* stat_sum,
                            float* stat_sq, int merge_F, int merge_K, const uint32_t* seed_base, void* stream);
int hwgat_linear_tn_bf16(const void* A, const void* B, float* dW, float* db, int64_t M, int N, int K,
                         uint32_t pro_seed, float pro_p, const float* mean, const float* rstd,
                         const float* gamma, const float* beta, const uint32_t* seed_base, void* stream);
/* The same for plain operands (no dropout mask, no LayerNorm) with a caller-owned workspace of
 * hwgat_linear_tn_bf16_ws_bytes(M, N, K) bytes: the partial dW tiles of the M slices are written as slabs and added in a
 * FIXED order by a second launch (no global atomics: ~20 us less per launch at the HWGAT shapes, dW bit-reproducible).
 * ws == NULL, too small, or a shape the slab kernel does not take (the query returns 0): hwgat_linear_tn_bf16. */
int64_t hwgat_linear_tn_bf16_ws_bytes(int64_t M, int N, int K);
int hwgat_linear_tn_bf16_ws(const void* A, const void* B, float* dW, float* db, int64_t M, int N, int K,
                            float* ws, int64_t ws_bytes, void* stream);

/* Bit-reproducible weight / bias gradients (round 4): the same kernels as hwgat_linear_tn_f32 / _bf16 (any prologue), but
 * the block of M split s STORES its partial dW tile and bias gradient into image s of the caller's ZERO-FILLED workspace
 * and one pass adds the images in split order -- no float atomics, the same bits on every run.  M % 32 == 0;
 * ws_bytes >= hwgat_linear_tn_det_bytes(M, N, K) (0: shape not supported).  Slower than the atomic / slab forms by the
 * workspace round trip; the reference's own single-device training is reproducible, this is the mode that matches it. */
int64_t hwgat_linear_tn_det_bytes(int64_t M, int N, int K);
int hwgat_linear_tn_f32_det(const float* A, const float* B, float* dW, float* db, int64_t M, int N, int K,
                            uint32_t pro_seed, float pro_p, const float* mean, const float* rstd,
                            const float* gamma, const float* beta, const uint32_t* seed_base, float* ws,
                            int64_t ws_bytes, void* stream);
int hwgat_linear_tn_bf16_det(const void* A, const void* B, float* dW, float* db, int64_t M, int N, int K,
                             uint32_t pro_seed, float pro_p, const float* mean, const float* rstd,
                             const float* gamma, const float* beta, const uint32_t* seed_base, float* ws,
                             int64_t ws_bytes, void* stream);

/* hwgat_linear_tn_f32 with a caller-owned workspace of hwgat_linear_tn_f32_ws_bytes(M, N, K) bytes: where the 256x256-tile
 * kernel (N, K multiples of 256) or the whole-weight kernel of the narrow layers ((N, K) = (384,128), (256,128), (128,256),
 * (128,128); M % 32 == 0) takes the shape, the partial dW tiles of the M slices go to slabs and a
 * second launch adds them in a FIXED order instead of 64 MB of global float atomics (~25 us less per launch, dW
 * bit-reproducible).  Every argument as in hwgat_linear_tn_f32; ws == NULL, too small, or the query returned 0: identical
 * to hwgat_linear_tn_f32. */
int64_t hwgat_linear_tn_f32_ws_bytes(int64_t M, int N, int K);
int hwgat_linear_tn_f32_ws(const float* A, const float* B, float* dW, float* db, int64_t M, int N, int K,
                           uint32_t pro_seed, float pro_p, const float* mean, const float* rstd,
                           const float* gamma, const float* beta, float* ws, int64_t ws_bytes,
                           const uint32_t* seed_base, void* stream);

/* out[C,R] = in[R,C]^T (used on weights only) */
int hwgat_transpose_f32(const float* in, float* out, int R, int C, void* stream);

/* ---- per-step weight preparation: ONE launch makes every derived copy of the fp32 master weights the fused linears
 * consume, for all blocks of a model (no reference counterpart: operands of the kernels above).  `table` is an array of
 * `n` entries in DEVICE memory, sorted by first_block; entry i owns workgroups [first_block, next entry's first_block):
 *   op 0 copy:       out[N][K] = (dtype) W[N][K]                    ceil(N/32) * ceil(K/32) workgroups
 *   op 1 transpose:  out[K][N] = (dtype) W[N][K]^T                  ceil(N/32) * ceil(K/32) workgroups
 *   op 2 LN fold:    out = W o gamma (dtype), s[N], c[N] exactly as hwgat_ln_fold (bias may be NULL)   ceil(N/4) workgroups
 * total_blocks = the sum of the entries' workgroups; dtype = HWGAT_F32 | HWGAT_BF16 of every `out`. */
typedef struct {
    const float* W; const float* bias; const float* gamma; const float* beta;
    void* out; float* s; float* c;
    int32_t N, K, op, first_block;
} hwgat_prep_entry;
int hwgat_weight_prep(const hwgat_prep_entry* table, int n, int total_blocks, int dtype, void* stream);

/* ---- the optimizers: AdamW / Adam, SGD and NAdam for all parameter tensors of a model in one launch each (reference:
 * cfg.optimizer_type 'adamw' / 'adam' / 'sgd' / 'nadam' as hwgat/utils.py:71-84 builds them and utils.py:93-116 steps them;
 * torch.optim.AdamW / Adam with amsgrad = maximize = False, torch.optim.SGD and torch.optim.NAdam with maximize = False).
 * Parameters, gradients and state are fp32.  Every value that changes between steps lives in DEVICE memory and is read
 * when the kernels run, so the advance and step launches below can be captured in a HIP graph and replayed under a
 * learning-rate schedule.  `kind` is one of HWGAT_OPT_ADAMW / HWGAT_OPT_SGD / HWGAT_OPT_NADAM; any other value is refused.
 *
 * table: `n` hwgat_opt_entry records in DEVICE memory, sorted by first_block; entry i owns workgroups [first_block, next
 *   entry's first_block) of hwgat_opt_step, ceil(n_i / HWGAT_OPTIM_CHUNK) of them, workgroup b covering elements
 *   [b * CHUNK, min(n_i, (b + 1) * CHUNK)); `group` selects the hyper-parameter block.  s0 / s1 are the tensor's state
 *   arrays, w0 / w1 its own scalar device words:
 *     AdamW  s0 = exp_avg (m), s1 = exp_avg_sq (v), w0 = step count, one fp32 device word (torch's state["step"] of a
 *            capturable optimizer); w1 = NULL.
 *     SGD    s0 = momentum buffer, w0 = "stepped before" word (0.0f = never, anything else = yes); s1 = w1 = NULL.
 *            s0 = w0 = NULL for a tensor of a group without momentum: nothing but p and g is touched then.
 *     NAdam  s0 = exp_avg, s1 = exp_avg_sq, w0 = step count, w1 = mu_product (torch's state["step"] and
 *            state["mu_product"] of a capturable NAdam); all four required.
 *   A tensor whose p, g and state arrays are all 16-byte aligned moves in 16-byte vectors, any other (e.g. a gradient that
 *   is a view into a flat bucket) element by element; both give the same bits.
 * hyper: HWGAT_OPTIM_NHYPER fp64 words per group:
 *     AdamW  { lr, beta1, beta2, eps, weight_decay, coupled (0 = AdamW, decoupled decay; 1 = Adam, decay added to the
 *              gradient), 0, 0 }
 *     SGD    { lr, momentum, dampening, weight_decay, nesterov (0 / 1), 0, 0, 0 }
 *     NAdam  { lr, beta1, beta2, eps, weight_decay, coupled (0 = decoupled decay, 1 = decay added to the gradient),
 *              momentum_decay, 0 }
 * derived: HWGAT_OPT_NDERIVED fp32 words per table entry, scratch that hwgat_opt_advance writes and hwgat_opt_step reads:
 *   the per-tensor scalars of the update rounded from fp64 once.
 * guard_state: NULL, or the state block of a gradient guard (below).  With one, advance and step return at once when its
 *   `skip` word is set, so no step count, "stepped" word, mu_product, parameter or state element is written.  It is the
 *   only pointer of these entry points that may be NULL; the kernels launched without one take no such argument.
 *
 * hwgat_opt_set:     one thread writes group `group` of `hyper` from the HWGAT_OPTIM_NHYPER HOST doubles at `values`, in the
 *                    layout of `kind` above.  They travel as a kernel argument (no copy, no copy node; stream-ordered like
 *                    hwgat_seed_set): `values` is not read after the call returns.
 * hwgat_opt_advance: one thread per entry, in fp64, the entry's derived block from its group's hyper block.  A launch of
 *                    its own: the workgroups of one entry must all see the same t.
 *                      AdamW  *w0 += 1 (t); lr wd, wd, 1 - beta1, beta2, 1 - beta2, lr / (1 - beta1^t), sqrt(1 - beta2^t), eps.
 *                      SGD    when the group's momentum != 0 and the entry has a buffer, first = (*w0 == 0), then *w0 = 1;
 *                             lr, weight_decay, momentum, 1 - dampening, flags.
 *                      NAdam  t = *w0 + 1, *w0 = t; mu = beta1 (1 - 0.5 * 0.96^(t momentum_decay)), mu' the same at t + 1;
 *                             *w1 = (float)(*w1 * mu); then the entry's fp32 scalars, among them 1 - beta2^t,
 *                             cg = lr (1 - mu) / (1 - *w1) and cm = lr mu' / (1 - *w1 mu').
 * hwgat_opt_step:    for each element, in fp32 (fused multiply-adds as written, nothing else contracted):
 *                      AdamW  p = p - (lr wd) p                       AdamW   |   g = g + wd p    Adam
 *                             m = m + (1 - beta1) (g - m)
 *                             v = ((1 - beta2) g) g + beta2 v
 *                             p = p - (lr / (1 - beta1^t)) (m / (sqrt(v) / sqrt(1 - beta2^t) + eps))
 *                      SGD    g' = g + wd p
 *                             with a buffer:   buf = first ? g' : (1 - dampening) g' + momentum buf   (a select: the old
 *                                              contents of a never-stepped buffer are not used, as torch clones the gradient)
 *                                              d = nesterov ? g' + momentum buf : buf
 *                             without:         d = g'
 *                             p = p - lr d
 *                             12 bytes per element without a buffer, 20 with one.
 *                      NAdam  p = p - (lr wd) p                       decoupled   |   g = g + wd p    coupled
 *                             m = m + (1 - beta1) (g - m)
 *                             v = ((1 - beta2) g) g + beta2 v
 *                             denom = sqrt(v / (1 - beta2^t)) + eps
 *                             p = p - cg (g / denom);   p = p - cm (m / denom)
 *                             28 bytes per element, as for AdamW.
 *                    total_blocks = the sum of the entries' workgroups.  No atomics, no reductions: bit-reproducible. */
#define HWGAT_OPTIM_CHUNK 4096
#define HWGAT_OPTIM_NHYPER 8
#define HWGAT_OPT_NDERIVED 16
enum { HWGAT_OPT_ADAMW = 0, HWGAT_OPT_SGD = 1, HWGAT_OPT_NADAM = 2 };
typedef struct {
    float* p; const float* g; float* s0; float* s1; float* w0; float* w1;
    int64_t n;
    int32_t group, first_block;
} hwgat_opt_entry;
int hwgat_opt_set(double* hyper, int group, int kind, const double* values, void* stream);
int hwgat_opt_advance(int kind, const hwgat_opt_entry* table, int n, const double* hyper, float* derived,
                      const double* guard_state, void* stream);
int hwgat_opt_step(int kind, const hwgat_opt_entry* table, int n, const float* derived, int total_blocks,
                   const double* guard_state, void* stream);

/* ---- gradient guard: clip all gradients of a model by their global norm (torch.nn.utils.clip_grad_norm_, norm_type 2 or
 * inf) and turn a step whose gradients hold a NaN or an Inf into a no-op, with every result left in DEVICE memory: nothing
 * is read back to the host, so the launches below can be captured in a HIP graph together with the optimizer step.
 *
 * table: the optimizer's own table, `n` hwgat_opt_entry records in DEVICE memory; only `g`, `n` and `first_block` of a
 *   record are used.  Workgroups are assigned as for hwgat_opt_step: one workgroup of 256 threads per HWGAT_OPTIM_CHUNK
 *   elements of one tensor.
 * state: HWGAT_GGUARD_NSTATE fp64 words in DEVICE memory, at the HWGAT_GGUARD_* slots below.  The three config words are
 *   written by hwgat_gguard_set, the others by hwgat_gguard_finish; the caller zeroes the block once.
 * workspace: 2 * total_blocks fp64 words in DEVICE memory: per workgroup { partial, flags (1 = saw a NaN, 2 = saw an Inf) }.
 *
 * hwgat_gguard_set:     one thread writes max_norm (>= 0, +Inf = measure only), norm_type (2 or +Inf) and the mode
 *                       (skip != 0: a step with a non-finite gradient is skipped; 0: it propagates, as in torch) from the
 *                       host values given as arguments; stream-ordered like hwgat_opt_set.
 * hwgat_gguard_partial: per workgroup the sum of g^2 in fp64 (norm_type 2) or max |g| (norm_type Inf) over its chunk:
 *                       per thread in a fixed element order, then in-wave, then across the four waves through LDS, in a
 *                       fixed order; one 16-byte store per workgroup, no atomics.  A 16-byte-aligned tensor moves in
 *                       16-byte vectors, any other element by element; both give every thread the same elements in the
 *                       same order, hence the same bits.
 * hwgat_gguard_finish:  one workgroup folds the partials in a fixed order and writes, in fp64:
 *                         total_norm = sqrt(sum) | max (NaN when a NaN was seen);
 *                         clip_coef  = c < 1 or c is NaN ? c : 1,   c = max_norm / (total_norm + 1e-6)   (torch's formula);
 *                         nonfinite  = a NaN or an Inf was seen;   skip = nonfinite && mode == skip;
 *                         steps += 1;  clipped += (clip_coef < 1 && !skip);  skipped += skip.
 * hwgat_gguard_scale:   g = g * (float)clip_coef in place for every element of every entry (also when clip_coef == 1: the
 *                       bits do not change); writes nothing when `skip` is set.  8 bytes per element.
 * hwgat_opt_advance / hwgat_opt_step take the state block as `guard_state` and do nothing when `skip` is set. */
#define HWGAT_GGUARD_NSTATE 16
#define HWGAT_GGUARD_MAX_NORM 0
#define HWGAT_GGUARD_NORM_TYPE 1
#define HWGAT_GGUARD_MODE 2
#define HWGAT_GGUARD_TOTAL_NORM 3
#define HWGAT_GGUARD_CLIP_COEF 4
#define HWGAT_GGUARD_NONFINITE 5
#define HWGAT_GGUARD_SKIP 6
#define HWGAT_GGUARD_STEPS 7
#define HWGAT_GGUARD_CLIPPED 8
#define HWGAT_GGUARD_SKIPPED 9
int hwgat_gguard_set(double* state, double max_norm, double norm_type, int skip, void* stream);
int hwgat_gguard_partial(const hwgat_opt_entry* table, int n, const double* state, double* workspace, int total_blocks,
                         void* stream);
int hwgat_gguard_finish(const double* workspace, int total_blocks, double* state, void* stream);
int hwgat_gguard_scale(const hwgat_opt_entry* table, int n, const double* state, int total_blocks, void* stream);

/* ---- weight averaging: an exponential moving average (EMA) or the equal-weight running mean (SWA) of the weights, as
 * torch.optim.swa_utils.AveragedModel keeps it, with every number left in DEVICE memory, so the launches below can be
 * captured in a HIP graph behind the optimizer step; and the in-place exchange of the averages with the live weights.
 *
 * table: `n` hwgat_wavg_entry records (HWGAT_WAVG_ENTRY_BYTES each) in DEVICE memory, sorted by first_block, workgroups
 *   assigned as for hwgat_opt_step: one workgroup of 256 threads per HWGAT_OPTIM_CHUNK elements of one tensor.  avg and
 *   src are fp32, 4-byte aligned and must not overlap.  A tensor whose avg and src are both 16-byte aligned moves in 16-byte
 *   vectors, any other element by element; both give the same bits.
 * state: HWGAT_WAVG_NSTATE fp64 words in DEVICE memory, at the HWGAT_WAVG_* slots below.  The five config words are written
 *   by hwgat_wavg_set, the four result words by hwgat_wavg_advance; the caller zeroes the block once.
 *
 * hwgat_wavg_set:     one thread writes mode (0 = EMA, 1 = equal weight), decay (in [0, 1)), warmup (0 / 1), start (>= 0)
 *                     and every (>= 1) from the host values given as arguments; stream-ordered like hwgat_opt_set.
 * hwgat_wavg_advance: one thread.  guard_state (may be NULL) is a gradient guard's state block: when its `skip` word is
 *                     set, active = 0, coef = 0 and no counter moves.  Otherwise steps_seen += 1; the update is due when
 *                     steps_seen > start and (steps_seen - start) % every == 0.  Not due: active = 0.  Due: active = 1,
 *                       coef = 1                                           when n_averaged == 0 (the first update copies),
 *                       coef = 1 - d,  d = decay                           EMA
 *                                      d = min(decay, (1 + n_averaged) / (10 + n_averaged))   EMA with warmup
 *                       coef = 1 / (n_averaged + 1)                        equal weight
 *                     in fp64, then n_averaged += 1.
 * hwgat_wavg_update:  active == 0: writes nothing.  coef == 1: avg = src, the same bits.  Otherwise, per element in fp32,
 *                     avg = fma((float)coef, src - avg, avg).  src is only read.  12 bytes per element.  No atomics, no
 *                     reductions: bit-reproducible.
 * hwgat_wavg_swap:    exchanges avg[i] and src[i] for every element of every entry.  16 bytes per element. */
#define HWGAT_WAVG_NSTATE 16
#define HWGAT_WAVG_ENTRY_BYTES 32
#define HWGAT_WAVG_MODE 0
#define HWGAT_WAVG_DECAY 1
#define HWGAT_WAVG_WARMUP 2
#define HWGAT_WAVG_START 3
#define HWGAT_WAVG_EVERY 4
#define HWGAT_WAVG_STEPS_SEEN 5
#define HWGAT_WAVG_N_AVERAGED 6
#define HWGAT_WAVG_COEF 7
#define HWGAT_WAVG_ACTIVE 8
typedef struct {
    float* avg; float* src;
    int64_t n;
    int32_t first_block, pad;
} hwgat_wavg_entry;
int hwgat_wavg_set(double* state, int mode, double decay, int warmup, int64_t start, int64_t every, void* stream);
int hwgat_wavg_advance(double* state, const double* guard_state, void* stream);
int hwgat_wavg_update(const hwgat_wavg_entry* table, int n, const double* state, int total_blocks, void* stream);
int hwgat_wavg_swap(const hwgat_wavg_entry* table, int n, int total_blocks, void* stream);

/* ---- train meters: what the reference's train() reads back after every batch (utils.py:109-114: `loss.item()`, the
 * correct predictions) summed on the device instead, so a train step captured in a HIP graph needs no host read per batch;
 * one more launch behind the optimizer's (and the averager's), one read per epoch or later.
 *
 * block: hwgat_meter_bytes(log_capacity, history_capacity) bytes of DEVICE memory, 8-byte aligned, zeroed once by the
 *   caller, in 8-byte words:
 *     [0, HWGAT_METER_RUN)                 header, int64: HWGAT_METER_LOG_TOTAL (records ever appended to the log),
 *                                          HWGAT_METER_CLOSED (epochs closed), HWGAT_METER_OVERFLOW (closes that found the
 *                                          history full), one spare
 *     [HWGAT_METER_RUN, HWGAT_METER_LOG)   the running words of the open epoch: HWGAT_METER_NRUN words at the HWGAT_METER_R_*
 *                                          slots.  int64: steps, rows, correct, finite_steps, nonfinite_loss, skipped;
 *                                          fp64: loss_sum, max_grad_norm; fp32 in the word's low four bytes (the high four
 *                                          are zero): last_loss, max_loss
 *     [HWGAT_METER_LOG, + 2 log_capacity)  the step log, a ring of 16-byte records { float loss; int32 correct; int32 rows;
 *                                          float grad_norm }: record number r (from 0) sits in slot r % log_capacity, so
 *                                          the ring holds the latest min(LOG_TOTAL, log_capacity) of them
 *     [.., + NRUN history_capacity)        the closed epochs, HWGAT_METER_NRUN words each, a copy of the running words
 *
 * hwgat_meter_fold:  one thread folds one step.  loss: the step's fp32 device word; correct: its int64 device word; n_rows:
 *                    its int32 device word with the real row count, or NULL: the constant batch_rows (>= 0) counts;
 *                    guard_state: a gradient guard's block (HWGAT_GGUARD_*), or NULL.
 *                      steps += 1; rows += n; correct += correct;
 *                      loss finite:  finite_steps += 1; loss_sum = loss_sum + (double)loss -- one IEEE addition per step in
 *                                    fold order, nothing fused: what Python's `total += loss.item()` gives, bit for bit;
 *                                    max_loss = the first finite loss of the epoch, then the larger;
 *                      otherwise:    nonfinite_loss += 1, loss_sum and max_loss untouched;
 *                      last_loss = loss (whatever it is);
 *                      guard: skipped += (skip word != 0); max_grad_norm = total_norm where total_norm > max_grad_norm (a
 *                             NaN norm never is, an Inf norm is);
 *                      log (log_capacity > 0): record { loss, (int32)correct, (int32)n, (float)total_norm or 0 },
 *                      LOG_TOTAL += 1.
 *                    No atomics, no reduction: every sum has one order.
 * hwgat_meter_close: copies the running words to history slot min(CLOSED, history_capacity - 1) (none when
 *                    history_capacity is 0), OVERFLOW += (CLOSED >= history_capacity), CLOSED += 1, zeroes the running
 *                    words; the step log and LOG_TOTAL stay. */
#define HWGAT_METER_LOG_TOTAL 0
#define HWGAT_METER_CLOSED 1
#define HWGAT_METER_OVERFLOW 2
#define HWGAT_METER_RUN 4
#define HWGAT_METER_NRUN 12
#define HWGAT_METER_LOG (HWGAT_METER_RUN + HWGAT_METER_NRUN)
#define HWGAT_METER_R_STEPS 0
#define HWGAT_METER_R_ROWS 1
#define HWGAT_METER_R_CORRECT 2
#define HWGAT_METER_R_LOSS_SUM 3
#define HWGAT_METER_R_FINITE_STEPS 4
#define HWGAT_METER_R_NONFINITE_LOSS 5
#define HWGAT_METER_R_SKIPPED 6
#define HWGAT_METER_R_LAST_LOSS 7
#define HWGAT_METER_R_MAX_LOSS 8
#define HWGAT_METER_R_MAX_GRAD_NORM 9
#define HWGAT_METER_MAX_CAPACITY (1 << 24)
int64_t hwgat_meter_bytes(int log_capacity, int history_capacity);
int hwgat_meter_fold(int64_t* block, const float* loss, const int64_t* correct, const int32_t* n_rows, int batch_rows,
                     const double* guard_state, int log_capacity, void* stream);
int hwgat_meter_close(int64_t* block, int log_capacity, int history_capacity, void* stream);

/* the dropout mask the fused kernels use: out[i] = keep(seed, i) ? 1/(1-p) : 0 */
int hwgat_dropout_mask_f32(float* out, int64_t n, uint32_t seed, float p, const uint32_t* seed_base, void* stream);

/* ---- device-side train / val-test transforms (reference hwgat/configs.py:93-108; host half: sl-hwgat_amd/augment.py).
 * A batch of n_clips ragged raw clips is packed frame after frame: x (total_frames, J, C) fp32, C in {2, 3}, clip i
 * owning frames [clip_off[i], clip_off[i+1]) (clip_off: n_clips + 1 device int32, clip_off[0] = 0,
 * clip_off[n_clips] <= total_frames).
 *
 * hwgat_aug_hand_fill: KeypointMasking's zeroing + HandCorrection (dataTransform.py:236-253, 328-403) in place on x.
 *   masked   (total_frames) device uint8, 1 = the frame's hand joints are zeroed first; NULL = no masking (eval)
 *   hands    HOST int32[6] = {left first joint, left end joint, left wrist, right first, right end, right wrist}; two
 *            disjoint ranges of at most 32 / C joints, wrists outside both
 *   per (clip, hand): "present" = any coordinate of the hand's joints is non-zero (and the frame is not masked).  No
 *   present frame: every frame takes its wrist.  Otherwise frames before the first / after the last present frame take
 *   their wrist, and with >= 3 present frames every absent frame in between takes the value at that frame of the
 *   interpolating quadratic spline (scipy splrep(k=2, s=0) / splev) through the present frames, per joint and
 *   coordinate, solved in fp64 and rounded to fp32; with fewer the gaps stay zero (the reference's bare except).
 *   max_frames >= every clip length, <= HWGAT_AUG_MAX_FRAMES (LDS: 12 bytes per frame);
 *   ws: device workspace of >= hwgat_aug_hand_fill_ws_bytes(total_frames) bytes (fp64 elimination columns);
 *   tap: NULL, or (total_frames, J, C) fp64 receiving the unrounded spline values at the elements the spline writes.
 * hwgat_aug_resample: out (n_clips, src_len, J_out, C) fp32 =
 *   flip(rotate(shear(normalise(x[clip_off[b] + src[b][t], gather[k]])))) per clip b, in fp64 after a normalisation in
 *   fp32 (as the reference computes it), one rounding to fp32 at the end
 *   src      (n_clips, src_len) device int32 frame map into the clip (TemporalAugmentation + TemporalSample composed)
 *   gather   (J_out) device int32 raw joint per output slot (the 64-slot WindowCreate table: parts.part_table(29)),
 *            or NULL with J_out = J
 *   prm      (n_clips, HWGAT_AUG_NPRM) device fp64 per clip: [0..2] left_top (fp32 values), [3] edge_dist (fp32
 *            value), [4..6] shear origin, [7] shear, [8..10] rotation origin, [11..19] rotation matrix M, row-major
 *            3x3, applied as x @ M (C = 2: its upper-left 2x2), [20] flip (x0 -> 1 - x0) if non-zero, [21] non-zero:
 *            the flip is taken in fp32 of the rounded value (TemporalSample padded the clip into an fp32 buffer).
 *            Coordinates past C of the 3-vectors are ignored.  Eval: zero origins and shear, M = I, no flip. */
#define HWGAT_AUG_NPRM 24
#define HWGAT_AUG_MAX_FRAMES 4096
int64_t hwgat_aug_hand_fill_ws_bytes(int64_t total_frames);
int hwgat_aug_hand_fill(float* x, const int32_t* clip_off, const uint8_t* masked, int n_clips, int64_t total_frames,
                        int max_frames, int J, int C, const int32_t* hands, void* ws, int64_t ws_bytes, double* tap,
                        void* stream);
int hwgat_aug_resample(const float* x, const int32_t* clip_off, const int32_t* src, const double* prm,
                       const int32_t* gather, float* out, int n_clips, int src_len, int J, int J_out, int C,
                       void* stream);

/* ---- streaming recognition (serve.StreamRecognizer): n_streams keypoint streams kept in device ring buffers, cut into the
 * packed clip / frame map / parameter record that hwgat_aug_hand_fill and hwgat_aug_resample take (the eval transform of
 * augment.EvalTransform.draw, normalisation included), and a decision rule behind the logits.  Every value that changes
 * between steps is a DEVICE word, so push -> window -> hand fill -> resample -> forward -> decide replays as one HIP graph.
 *
 * ring:  (n_streams, ring_frames, J, C) fp32 raw frames, ring_frames <= HWGAT_AUG_MAX_FRAMES, C in {2, 3}.
 * state: hwgat_stream_state_bytes(n_streams, log_capacity) bytes of DEVICE memory, 8-byte aligned, zeroed once by the caller
 *        (the four hyper-parameter words are then written by the caller):
 *          hwgat_stream_header                       log_count: events in the log; overflow: events that found it full;
 *                                                    alpha, threshold, hold, blank_class: the decision rule's parameters,
 *                                                    read when hwgat_stream_decide runs
 *          hwgat_stream_words[n_streams]             per stream, see the struct
 *          hwgat_stream_event[log_capacity]          the event log, in the order the events were emitted
 *
 * hwgat_stream_push: appends n = clamp(n_new[s], 0, push_frames) frames of frames (n_streams, push_frames, J, C) to ring s at
 *   slot head, head + 1, .. (mod ring_frames), overwriting the oldest; head = (head + n) mod ring_frames,
 *   count = min(count + n, ring_frames), frames_seen += n.  push_frames <= ring_frames.  head and count are reduced to
 *   [0, ring_frames) / [0, ring_frames] when they are read, so no word of device memory can move an address out of the ring.
 * hwgat_stream_window: per stream, L = min(count, window_frames) (window_frames <= ring_frames):
 *   clip      (n_streams * window_frames, J, C) fp32: the L newest frames, oldest first, stream after stream
 *   clip_off  (n_streams + 1) int32 prefix sums of L
 *   src       (n_streams, src_len) int32: EvalTransform._temporal_sample(L, False).  L <= src_len: centred, padded with the
 *             first frame in the front half and the last behind; else int(i * ((L - 1) / (src_len - 1))) in fp64 with the last
 *             entry L - 1 (numpy.linspace(0, L - 1, src_len).astype(int)).  L = 0: zeros.
 *   prm       (n_streams, HWGAT_AUG_NPRM) fp64 eval record: [0..C) left_top, [3] edge_dist, M = I, [21] = (L <= src_len).
 *             From the first frame f of the window whose joints origin, anchor0, anchor1 are non-zero in every coordinate, in
 *             fp32, every operation rounded on its own: unit = sqrt(sum_c (kp[anchor0][c] - kp[anchor1][c])^2),
 *             left_top[c] = kp[origin][c] - 3 unit, left_top[1] = kp[origin][1] - 2 unit, edge_dist = 6 unit.
 *   ready     (in hwgat_stream_words) = count >= min_frames and such a frame exists and unit is positive and finite;
 *             otherwise the record is left_top = 0, edge_dist = 1.  A stream without frames has an empty clip, which both
 *             transform kernels take (the hand fill returns, the resampler writes zeros).
 *   hands     HOST int32[6] as for hwgat_aug_hand_fill; origin and the anchors must lie in [0, J) outside both hands.
 * hwgat_stream_decide: per ready stream s, from logits (n_streams, n_classes) fp32 and q (n_streams, n_classes) fp32:
 *   p = softmax(logits[s]); q[s] = p on the stream's first ready evaluation, else (1 - alpha) q[s] + alpha p;
 *   top = lowest arg-max of q[s], conf = q[s][top]; run = run + 1 if top is the previous top, else run = 1 and fired = 0;
 *   run >= hold and conf >= threshold and fired == 0 and top != blank_class: an event { s, frames_seen, evals, top, conf } is
 *   appended (or counted in overflow when log_count == log_capacity) and fired = 1; then evals += 1.
 *   One workgroup: a wave per stream, each sum in one fixed order, the log appended by one thread in stream order.  A stream
 *   that is not ready is not touched. */
#define HWGAT_STREAM_MAX_STREAMS 64
#define HWGAT_STREAM_MAX_CLASSES 65536
#define HWGAT_STREAM_MAX_LOG (1 << 20)
typedef struct {
    int64_t log_count, overflow;
    float alpha, threshold;
    int32_t hold, blank_class;                  /* blank_class -1: none */
    int64_t spare[4];
} hwgat_stream_header;                          /* 64 bytes */
typedef struct {
    int32_t head, count;                        /* next slot to write; frames held, <= ring_frames */
    int64_t frames_seen;                        /* frames ever pushed */
    int32_t ready, win_len;                     /* of the last hwgat_stream_window: ready word, L */
    int32_t top, run;                           /* of the last ready evaluation */
    float conf;
    int32_t fired;
    int64_t evals, events;                      /* ready evaluations; events emitted (overflowed ones included) */
    int64_t spare;
} hwgat_stream_words;                           /* 64 bytes */
typedef struct {
    int64_t frames_seen, evaluation;            /* the stream's frames_seen and 0-based ready evaluation at the event */
    int32_t stream, cls;
    float conf;
    int32_t pad;
} hwgat_stream_event;                           /* 32 bytes */
int64_t hwgat_stream_state_bytes(int n_streams, int log_capacity);
int hwgat_stream_push(float* ring, void* state, const float* frames, const int32_t* n_new, int n_streams, int ring_frames,
                      int push_frames, int J, int C, void* stream);
int hwgat_stream_window(const float* ring, void* state, float* clip, int32_t* clip_off, int32_t* src, double* prm,
                        int n_streams, int ring_frames, int window_frames, int min_frames, int src_len, int J, int C,
                        int origin, int anchor0, int anchor1, const int32_t* hands, void* stream);
int hwgat_stream_decide(void* state, float* q, const float* logits, int n_streams, int n_classes, int log_capacity,
                        void* stream);

/* ---- device-resident clip store and train input pipeline (data.DeviceClipStore / data.DeviceLoader, csrc/loader.hip).
 * The whole dataset lives on the device; "the next batch" is hwgat_loader_select -> hwgat_loader_draw ->
 * hwgat_aug_hand_fill -> hwgat_aug_resample with no host input: every value that changes between batches is a DEVICE word,
 * so the four launches replay as one HIP graph.  The shuffle and the augmentation draw are counter-based hashes of a
 * device-resident seed, as dropout is.
 *
 * store (device memory, built once by the caller):
 *   frames    (store_frames, J, C) fp32: all raw clips one after another, C in {2, 3}
 *   clip_off  (n_clips + 1) int64 prefix sums of the clip lengths; every clip has 1..max_frames frames
 *   labels    (n_clips) int64
 *   norm      (n_clips, 4) fp32: left_top[0..2], edge_dist of NormalizeKeypoints (fp32 values computed once on the host from
 *             the raw clip: the origin and anchor joints are never masked or hand-corrected)
 * state: hwgat_loader_state_bytes() = 64 bytes of DEVICE memory, 8-byte aligned (hwgat_loader_state), written by the caller.
 *   Every word is reduced to its range when a kernel reads it -- n_clips to [1, n_clips argument], batch to [1, batch
 *   argument], world to [1, 2^20], rank to [0, world), cursor to [0, batches per epoch), clip ids to [0, n_clips), clip
 *   offsets and lengths to the store, frame numbers to [0, T) -- so no word of device memory can move an address out of
 *   the store or the batch buffers.
 *
 * hashes.  mix32(seed, pair) is the dropout hash of csrc/fused_ops.h (32-bit wrap-around arithmetic):
 *     x = ((uint32)pair ^ seed) * 0x9E3779B1 + (uint32)(pair >> 32) * 0x85EBCA77;
 *     x ^= x >> 15; x *= 0x2C1B3C6D; x ^= x >> 12; x *= 0x297A2D39; return x ^ (x >> 15).
 *   feistel(K, n, x), a bijection of [0, 2^b): b = the smallest EVEN number >= 2 with 2^b >= n, h = b / 2, m = 2^h - 1;
 *     (L, R) = (x >> h, x & m); for j = 0, 1, 2, 3: (L, R) = (R, L ^ (mix32(K + j, R) & m)); result (L << h) | R.
 *   perm(K, n, x), a bijection of [0, n) for x in [0, n): n == 1: 0; else y = x; do y = feistel(K, n, y) while y >= n
 *     (cycle walking).  2^b < 4 n (else b - 2 would do), so a step lands in [0, n) with probability > 1/4 and the expected
 *     number of steps is below 4.  The walk is bounded by 2^b - n + 1 steps and falls through to y = x at the bound; the
 *     bound is never reached: feistel is a bijection of [0, 2^b), so the walk runs along the cycle through x, which comes
 *     back to x -- a point of [0, n) -- after visiting each other point at most once, and only 2^b - n points lie outside.
 *   K_perm = mix32(seed, epoch)                                  (pair = epoch, high word 0)
 *   K_row  = mix32(mix32(seed, 2^32 + epoch), id)                (pair = 2^32 + epoch, then pair = id): the draw key of clip
 *            `id` in `epoch`.  It depends on (seed, epoch, id) only -- not on the batch size, the row or the rank.
 *   hash(tag, i) = mix32(K_row + tag, i)  with the HWGAT_LOADER_TAG_* below (16 apart: a Feistel key uses tag .. tag + 3)
 *   U(tag, i) = (hash(tag, i) + 0.5) / 2^32  in fp64 (exact), in (0, 1)
 *   Z(tag, i) = sqrt(-2 ln U(tag, 2 i)) * cos(6.283185307179586 * U(tag, 2 i + 1))  (Box-Muller, fp64, each product rounded)
 *   normal(loc, scale, tag, i) = loc + scale * Z(tag, i);  clip01(v) = min(max(v, 0), 1)
 *
 * hwgat_loader_select: ONE workgroup.  From the state words (reduced as above): flags bit 0 shuffle, bit 1 drop_last, bit 2
 *   train.  per = drop_last ? n_clips / world : ceil(n_clips / world); nb0 = drop_last ? per / batch : ceil(per / batch);
 *   batches per epoch nb = max(nb0, 1); limit = drop_last ? nb0 * batch * world : n_clips.  Row r < batch (state word) takes
 *   sample s = (cursor * batch + r) * world + rank; s >= limit or r >= batch: the row is empty (id -1, key 0, no frames,
 *   label 0).  Otherwise id = shuffle ? perm(K_perm, n_clips, s) : s.  It writes, for the `batch` ARGUMENT rows:
 *     ids (batch) int32; keys (batch) uint32 = K_row; clip_len (batch) int32 = the clip's length (0 for an empty row);
 *     batch_off (batch + 1) int32 prefix sums of clip_len (an LDS scan); y (batch) int64 = labels[id]; *n_rows = the number
 *     of non-empty rows (they come first).
 *   Then cursor += 1, and at cursor == nb: cursor = 0, epoch += 1.
 * hwgat_loader_draw: one workgroup per row; T = the row's clip length, id / K_row its clip and key.  It writes
 *   clip     (batch * max_frames, J, C) fp32: the clip's raw frames at frame batch_off[r]
 *   masked   (batch * max_frames) uint8 at batch_off[r]: train: frame f is 1 iff perm(K_row + TAG_MASK, T, f) < int(mask_p * T)
 *            (a uniformly random subset of int(mask_p T) frames, as sorted(random.sample(range(T), m))), else 0; eval: 0
 *   prm      (batch, HWGAT_AUG_NPRM) fp64, the record hwgat_aug_resample takes: [0..3] = norm[id] (as doubles);
 *            train: [4 + c] = clip01(normal(0.5, 0.1, TAG_SHEAR_ORIGIN, c)), [7] = normal(0, shear_std, TAG_SHEAR, 0),
 *            [8 + c] = clip01(normal(0.5, 0.1, TAG_ROT_ORIGIN, c)) for c < C (0 beyond);
 *            C = 2: a = normal(0, rotation_std, TAG_ROT, 0), M = [[cos a, -sin a, 0], [sin a, cos a, 0], [0, 0, 1]];
 *            C = 3: angles t_k = normal(0, rotation_std, TAG_ROT, k) * 90 * 0.017453292519943295 (radians), k = 0, 1, 2,
 *            M = Rz(t_2) Ry(t_1) Rx(t_0), extrinsic x-y-z (augment.euler_xyz_degrees):
 *              [[c2 c1, c2 s1 s0 - s2 c0, c2 s1 c0 + s2 s0], [s2 c1, s2 s1 s0 + c2 c0, s2 s1 c0 - c2 s0], [-s1, c1 s0, c1 c0]];
 *            [11 + 3 q + c] = M[q][c]; [20] = 1 iff hash(TAG_FLIP, 0) < 2^31; [21] = 1 iff L <= src_len (below); rest 0.
 *            eval: zero origins and shear, M = I, no flip, [21] = (T <= src_len).  Empty row: [3] = 1, M = I, rest 0.
 *   src      (batch, src_len) int32, the frame map src[i] = aug[m[i]] of TrainTransform.draw:
 *            ratio = (ratio_hi - ratio_lo) * U(TAG_RATIO, 0) + ratio_lo and L = int(T * ratio): a separately rounded fp64
 *            difference, product, sum and product (no FMA), L reduced to [1, 2 * HWGAT_AUG_MAX_FRAMES];
 *            random = random_sample and hash(TAG_MODE, 0) < 2^31.
 *            random, ratio <= 1: aug = the frames f with perm(K_row + TAG_SUBSET, T, f) < L in increasing order;
 *            random, ratio > 1: the L draws (hash(TAG_CHOICE, i) * T) >> 32 (64-bit product), i < L, sorted;
 *              (both: a count per frame in LDS -- integer atomics -- then an inclusive LDS scan; aug[j] is the first frame
 *              whose cumulative count exceeds j)
 *            else aug[j] = numpy.linspace(0, T - 1, L).astype(int)[j] = j == L - 1 ? T - 1 : int(j * ((T - 1) / (L - 1)))
 *              (fp64 quotient and product, each rounded; L == 1: 0).
 *            TemporalSample: L <= src_len: s = random_shift ? clip01(normal(0.5, 0.1, TAG_SHIFT, 0)) : 0.5,
 *            start = int((src_len - L) * s) (a rounded fp64 product); m[i] = i - start for start <= i < start + L, else 0 for
 *            i < src_len / 2 (integer division) and L - 1 behind; L > src_len: m[i] = linspace(0, L - 1, src_len).astype(int)[i].
 *            eval: L = T, aug[j] = j, s = 0.5.  Empty row: zeros.
 *   mask_p in (0, 1), 0 < ratio_lo <= ratio_hi <= 2 (so L <= 2 T), the standard deviations >= 0, else HWGAT_ESHAPE.
 *   LDS: one int32 counter per frame for HWGAT_AUG_MAX_FRAMES = 4096 frames (16 KiB), 256 scan partials (1 KiB), the
 *   normals and the record (0.4 KiB): under 18 KiB per workgroup.
 * Both: batch <= HWGAT_LOADER_MAX_BATCH, n_clips <= 2^30, max_frames <= HWGAT_AUG_MAX_FRAMES, batch * max_frames < 2^31,
 *   J <= 1024, src_len <= 2^20 (else HWGAT_ESHAPE).  No float atomics; every word has one writer; bit-reproducible.
 * The packed clip, batch_off, masked, src and prm then go to hwgat_aug_hand_fill / hwgat_aug_resample unchanged, with
 * n_clips = batch, total_frames = batch * max_frames (an empty row: the hand fill returns, the resampler writes zeros). */
#define HWGAT_LOADER_MAX_BATCH 1024
#define HWGAT_LOADER_SHUFFLE 1
#define HWGAT_LOADER_DROP_LAST 2
#define HWGAT_LOADER_TRAIN 4
#define HWGAT_LOADER_TAG_MASK 0x10
#define HWGAT_LOADER_TAG_SHEAR_ORIGIN 0x20
#define HWGAT_LOADER_TAG_SHEAR 0x30
#define HWGAT_LOADER_TAG_ROT_ORIGIN 0x40
#define HWGAT_LOADER_TAG_ROT 0x50
#define HWGAT_LOADER_TAG_RATIO 0x60
#define HWGAT_LOADER_TAG_MODE 0x70
#define HWGAT_LOADER_TAG_SUBSET 0x80
#define HWGAT_LOADER_TAG_CHOICE 0x90
#define HWGAT_LOADER_TAG_SHIFT 0xA0
#define HWGAT_LOADER_TAG_FLIP 0xB0
typedef struct {
    uint32_t seed, epoch;
    int32_t cursor, n_clips;                    /* batch within the epoch; clips in the store */
    int32_t batch, rank;
    int32_t world, flags;                       /* HWGAT_LOADER_SHUFFLE | _DROP_LAST | _TRAIN */
    int64_t spare[4];
} hwgat_loader_state;                           /* 64 bytes */
int64_t hwgat_loader_state_bytes(void);
int hwgat_loader_select(void* state, const int64_t* clip_off, const int64_t* labels, int32_t* ids, uint32_t* keys,
                        int32_t* clip_len, int32_t* batch_off, int64_t* y, int32_t* n_rows, int n_clips,
                        int64_t store_frames, int batch, int max_frames, void* stream);
int hwgat_loader_draw(const void* state, const float* frames, const int64_t* clip_off, const float* norm,
                      const int32_t* ids, const uint32_t* keys, const int32_t* batch_off, float* clip, uint8_t* masked,
                      int32_t* src, double* prm, int n_clips, int64_t store_frames, int batch, int max_frames, int src_len,
                      int J, int C, double mask_p, double ratio_lo, double ratio_hi, double shear_std, double rotation_std,
                      int random_sample, int random_shift, void* stream);

/* ---- Mixup and temporal CutMix of the pairs of a batch (train.BatchMixer, csrc/mix.hip).  Two launches in front of the
 * train step's forward mix the step's static input buffer in place: hwgat_mix_draw matches the batch's live rows into
 * pairs and draws every pair's decision, hwgat_mix_apply rewrites the rows.  Every value that changes between steps is
 * a DEVICE word of the mixer state, so both replay in a HIP graph.  Hashes, perm and U are the loader's (above).
 *
 * state: hwgat_mix_state_bytes() = 40 bytes of DEVICE memory, 8-byte aligned (hwgat_mix_state): seed, step (the replay
 *   counter), and the fp64 words prob, cutmix_share, mixup_alpha, cutmix_alpha.  The kernels reduce the alphas to
 *   [HWGAT_MIX_ALPHA_MIN, 1] when they read them.
 * hwgat_mix_set (one thread): writes the four hyper words from the host values given as arguments and, when
 *   `set_counter` is not 0, seed and step as well; stream-ordered like hwgat_opt_set.  prob and cutmix_share outside
 *   [0, 1] or an alpha outside [HWGAT_MIX_ALPHA_MIN, 1] (a NaN included) is HWGAT_ESHAPE.
 *
 * hwgat_mix_draw: ONE workgroup.  n = clamp(*n_rows, 0, B), a NULL n_rows means B.  With seed and step of the state:
 *     K_step = mix32(seed, HWGAT_MIX_TAG * 2^32 + step)      (the loader's keys use the high words 0 and 1)
 *     K_sigma = mix32(K_step, 0);   K_p = mix32(K_step, 1 + p), the key of pair p
 *     U_p(tag, i) = (mix32(K_p + tag, i) + 0.5) / 2^32  in fp64 (exact), with the HWGAT_MIX_TAG_* below
 *   matching: pair p < n / 2 (integer division) is the rows a = perm(K_sigma, n, 2 p) and b = perm(K_sigma, n, 2 p + 1): a
 *     uniformly keyed perfect matching of the live rows.  With n odd the row perm(K_sigma, n, n - 1) has no partner; nor
 *     has any row >= n.
 *   per pair: mixed iff U_p(TAG_APPLY, 0) < prob; then CutMix iff U_p(TAG_MODE, 0) < cutmix_share, else Mixup;
 *     alpha = cutmix_alpha or mixup_alpha accordingly; lambda0 ~ Beta(alpha, alpha) by Joehnk's method in fp64: for
 *     k = 0 .. 63: X = pow(U_p(TAG_BETA, 2 k), 1 / alpha), Y = pow(U_p(TAG_BETA, 2 k + 1), 1 / alpha) (1 / alpha a rounded
 *     fp64 quotient), S = X + Y; the first k with 0 < S <= 1 gives lambda0 = X / S; none in 64 tries: lambda0 = 0.5 (the
 *     acceptance probability Gamma(alpha + 1)^2 / Gamma(2 alpha + 1) is at least 1/2 for alpha <= 1: the fallback has
 *     probability <= 2^-64 and only bounds the loop; alpha >= 0.05 keeps U^(1 / alpha) >= 2^-640 above the denormals).
 *     Mixup:  lambda = (float)lambda0, seg = (0, 0).
 *     CutMix: L = clamp(floor((1 - lambda0) * T + 0.5), 0, T) (a rounded fp64 difference, product and sum: no FMA),
 *             t0 = min(floor(U_p(TAG_START, 0) * (T - L + 1)), T - L), lambda = (float)((double)(T - L) / T), seg = (t0, L).
 *   records, for every row r < B:
 *     partner (B) int32   the other row of r's pair when the pair is mixed, else r
 *     lam     (B) fp32    the pair's lambda for both of its rows; 1.0f when not mixed
 *     seg     (B, 2) int32  (t0, L) of a CutMix pair for both rows, else (0, 0)
 *     mode    (B) int32   HWGAT_MIX_NONE / HWGAT_MIX_MIXUP / HWGAT_MIX_CUTMIX
 *     y_b     (B) int64   y[partner[r]]   (y (B) int64 is only read; y_b must not overlap it)
 *   pairs (max(B / 2, 1), 2) int32: (a, b) for p < n / 2, (-1, -1) behind.  Every word has one writer.  After a workgroup
 *   barrier one thread does step += 1 (32-bit wrap).
 *   1 <= B <= HWGAT_MIX_MAX_BATCH, 1 <= T <= 2^20, else HWGAT_ESHAPE.
 *
 * hwgat_mix_apply: x (B, T, R) fp32 contiguous, R the product of the trailing dims; in place.  Pair p < n / 2 with rows
 *   (a, b) = pairs[p] -- a pair with a row outside [0, n) or a == b is skipped -- and mode[a]:
 *     Mixup:  w = fsub_rn(1, lambda); every element:  a' = fadd_rn(fmul_rn(lambda, a), fmul_rn(w, b)),
 *             b' = fadd_rn(fmul_rn(lambda, b), fmul_rn(w, a)): separately rounded fp32 products and sum, no FMA.
 *     CutMix: frames [t0, t0 + L) of the two rows are swapped ((t0, L) = seg[a] reduced to 0 <= t0 <= T, 0 <= L <= T - t0);
 *             no other element is read or written.
 *     none:   the pair is not touched; nor is any row >= n or the unpaired row.
 *   A pair is symmetric, so one thread reads an element of both rows and writes both: each element has one reader and
 *   one writer, which is what makes the in-place form safe.  16-byte accesses where both rows' segments share their
 *   alignment (always when T * R % 4 == 0) with a scalar head and tail up to the 16-byte boundaries, scalar throughout
 *   otherwise.  No atomics; bit-reproducible.  1 <= B <= HWGAT_MIX_MAX_BATCH, 1 <= T <= 2^20,
 *   1 <= R, T * R < 2^31, else HWGAT_ESHAPE. */
#define HWGAT_MIX_MAX_BATCH 65536
#define HWGAT_MIX_ALPHA_MIN 0.05
#define HWGAT_MIX_TAG 2
#define HWGAT_MIX_TAG_APPLY 0x10
#define HWGAT_MIX_TAG_MODE 0x20
#define HWGAT_MIX_TAG_BETA 0x30
#define HWGAT_MIX_TAG_START 0x40
#define HWGAT_MIX_NONE 0
#define HWGAT_MIX_MIXUP 1
#define HWGAT_MIX_CUTMIX 2
typedef struct {
    uint32_t seed, step;
    double prob, cutmix_share, mixup_alpha, cutmix_alpha;
} hwgat_mix_state;                              /* 40 bytes */
int64_t hwgat_mix_state_bytes(void);
int hwgat_mix_set(void* state, double prob, double cutmix_share, double mixup_alpha, double cutmix_alpha, int set_counter,
                  uint32_t seed, uint32_t step, void* stream);
int hwgat_mix_draw(void* state, const int64_t* y, const int32_t* n_rows, int32_t* pairs, int32_t* partner, float* lam,
                   int32_t* seg, int32_t* mode, int64_t* y_b, int B, int T, void* stream);
int hwgat_mix_apply(float* x, const int32_t* pairs, const float* lam, const int32_t* seg, const int32_t* mode,
                    const int32_t* n_rows, int B, int T, int64_t R, void* stream);

/* ---- Transformer baseline (ABI 4004; reference hwgat/models/Transformer.py).  Activations (B, T, d) with d = nH * 64.
 *
 * hwgat_seq_attn_fwd: multi-head attention of nn.MultiheadAttention(batch_first=True) with a key-padding mask over the
 *   T <= 512 frames of each clip, head_dim 64 (else HWGAT_ESHAPE).
 *   qkv  (B, T, 3d) in the in_proj layout (q | k | v, head h at columns h*64 .. h*64+63 of each third), `dtype`
 *   o    (B, T, d) out: softmax(q k^T / 8 + mask) v per head, head h at columns h*64 ..
 *   lse  (B, nH, T) fp32 out (may be NULL in eval): log-sum-exp of each query row, -inf for a query without a visible key
 *   pad  (B, ceil(T / 32)) uint32: bit t % 32 of word t / 32 set = frame t of the clip is padding (hwgat_seq_embed_fwd)
 *   A query whose keys are ALL padded gets o = 0 (torch 2.10 semantics).  Attention dropout (p in [0, 1)): the keep mask
 *   of probability (b, h, i, j) is the common hash of seed + *seed_base at index ((b nH + h) T + i) T + j, i.e. what
 *   hwgat_dropout_mask_f32 writes for a (B, nH, T, T) tensor.
 * hwgat_seq_attn_bwd: dqkv (B, T, 3d) of the same attention from o, dout = dL/do and the forward's lse; every element of
 *   dqkv is written (zero for padded keys and for queries without a visible key).  D: (B, nH, T) fp32 workspace.  Two
 *   launches, no atomics: bit-reproducible. */
int hwgat_seq_attn_fwd(const void* qkv, void* o, float* lse, const uint32_t* pad, int B, int T, int n_heads,
                       int head_dim, int dtype, uint32_t seed, float p, const uint32_t* seed_base, void* stream);
int hwgat_seq_attn_bwd(const void* qkv, const void* o, const void* dout, const float* lse, const uint32_t* pad,
                       void* dqkv, float* D, int B, int T, int n_heads, int head_dim, int dtype, uint32_t seed,
                       float p, const uint32_t* seed_base, void* stream);

/* hwgat_seq_embed_fwd: out (B, T, d) `dtype` = dropout((x Wt + bias) * sqrt(d) + pe[t]) (reference Transformer.py:
 *   encoder, * sqrt(d_model), PositionalEncoding) and pad (B, ceil(T / 32)) uint32 key-padding words, bit set iff
 *   x[b, t, 0] == pad_index (exact compare), in one launch.  x (B, T, F) fp32 with F <= 512 any width, Wt (F, d) fp32 =
 *   the encoder weight transposed, bias (d) or NULL, pe (T, d) fp32 or NULL; dropout mask index (b T + t) d + n.
 * hwgat_seq_embed_bwd: dW (d, F) += g^T x, db (d) += column sums of g (db may be NULL), g = dout * mask * sqrt(d)
 *   with the forward's (seed, p) over M = B T rows; ws: >= hwgat_seq_embed_bwd_bytes(F, d) bytes of device memory (need
 *   not be zeroed).  Fixed-order split sums, no atomics: bit-reproducible.
 * hwgat_seq_maxpool_fwd: out (B, d) fp32 = max over T of x (B, T, d) `dtype`, idx (B, d) int32 = first index of the
 *   maximum (torch.max).  hwgat_seq_maxpool_bwd: dx (B, T, d) `dtype` = dout at idx, 0 elsewhere. */
int hwgat_seq_embed_fwd(const float* x, const float* Wt, const float* bias, const float* pe, void* out, uint32_t* pad,
                        int B, int T, int F, int d, float pad_index, int dtype, uint32_t seed, float p,
                        const uint32_t* seed_base, void* stream);
int64_t hwgat_seq_embed_bwd_bytes(int F, int d);
int hwgat_seq_embed_bwd(const void* dout, const float* x, float* dW, float* db, int64_t M, int F, int d, int dtype,
                        uint32_t seed, float p, const uint32_t* seed_base, float* ws, int64_t ws_bytes, void* stream);
int hwgat_seq_maxpool_fwd(const void* x, float* out, int32_t* idx, int B, int T, int d, int dtype, void* stream);
int hwgat_seq_maxpool_bwd(const float* dout, const int32_t* idx, void* dx, int B, int T, int d, int dtype, void* stream);

/* ---- ST-GCN baseline (ABI 4005; reference hwgat/models/STGCN.py).  fp32 only.  Activations are channels-last
 * (N, T, V, C): M = N T V rows of C floats, a BatchNorm channel is a column.  No kernel of this group uses an atomic:
 * every cross-block sum goes through partial images added in a fixed order, so every result is bit-reproducible.
 *
 * Convolutions.  All three convolutions of a block (1x1 graph-conv projection, 9x1 temporal, strided 1x1 residual) are
 * one implicit GEMM: output row (n, t, v), reduction over taps x Cin, tap k reading input frame stride * t + k - pad of
 * the same clip and joint, zero outside [0, Tin).  Cin (as passed) a multiple of 32, Cout a multiple of 32, taps 1..9,
 * stride 1 or 2, Tout = (Tin + 2 pad - taps) / stride + 1 (else HWGAT_ESHAPE).
 * hwgat_stgcn_weight_prep: W (Cout, Cin, taps, 1) master -> out, mode 0: [tap][ci < CinP][co] (rows ci >= Cin zero),
 *   mode 1: [tap][co][ci < CinP].
 * hwgat_stgcn_conv: mode 0: out (Nc, Tout, V, Cout) = conv(in (Nc, Tin, V, Cin); wk = mode-0 image) + bias.
 *   mode 1: the input gradient: in = dL/dy (Nc, Tin = frames of y, V, Cin = channels of y), wk = mode-1 image,
 *   out (Nc, Tout = frames of x, V, Cout = channels of x, padded).  bias, add, mask may be NULL;
 *   out += add, or += add * [mask > 0] when mask is given (both shaped like out).
 * hwgat_stgcn_conv_dw: dW (Cout, Cin, taps, 1) = sum_m dy[m][co] in[src(m, tap)][ci] (written, not accumulated);
 *   in has CinP >= Cin channels per row (CinP a multiple of 32); ws >= hwgat_stgcn_conv_dw_bytes(Nc Tout V, CinP, Cout,
 *   taps) bytes, need not be zeroed. */
int hwgat_stgcn_weight_prep(const float* W, float* out, int Cout, int Cin, int taps, int CinP, int mode, void* stream);
int hwgat_stgcn_conv(const float* in, const float* wk, const float* bias, const float* add, const float* mask,
                     float* out, int Nc, int Tin, int Tout, int V, int Cin, int Cout, int taps, int stride, int pad,
                     int mode, void* stream);
int64_t hwgat_stgcn_conv_dw_bytes(int64_t M, int CinP, int Cout, int taps);
int hwgat_stgcn_conv_dw(const float* in, const float* dy, float* dW, int Nc, int Tin, int Tout, int V, int CinP, int Cin,
                        int Cout, int taps, int stride, int pad, float* ws, int64_t ws_bytes, void* stream);

/* Column reductions and BatchNorm over M rows of C columns.  ws: >= hwgat_stgcn_red_bytes(C) bytes, need not be zeroed.
 * hwgat_stgcn_colsum: out (C) = column sums of x (a convolution's bias gradient).
 * hwgat_stgcn_bn_stats: mean, rstd = 1 / sqrt(biased variance + eps) of every column (shifted sums: exact for a mean far
 *   above the deviation); running_mean / running_var (both or neither) <- (1 - momentum) old + momentum (mean, unbiased
 *   variance), *num_batches += 1 (int64, may be NULL), all on the device.  M < 2: HWGAT_ESHAPE.
 * hwgat_stgcn_bn_eval_stats: mean = running_mean, rstd = 1 / sqrt(running_var + eps).
 * hwgat_stgcn_bn_apply: out = (x - mean) rstd gamma + beta (+ res, itself normalised with the res_* set when res_mean is
 *   given), then max(., 0) if relu.
 * hwgat_stgcn_bn_bwd: g = dy, or dy [y > 0] when y (the forward's ReLU output) is given; dbeta = sum g, dgamma = sum g xhat
 *   (written); dx = gamma rstd (g - (dbeta + xhat dgamma) / M) with train != 0, gamma rstd g with running statistics. */
int64_t hwgat_stgcn_red_bytes(int C);
int hwgat_stgcn_colsum(const float* x, float* out, int64_t M, int C, float* ws, int64_t ws_bytes, void* stream);
int hwgat_stgcn_bn_stats(const float* x, int64_t M, int C, float eps, float momentum, float* mean, float* rstd,
                         float* running_mean, float* running_var, int64_t* num_batches, float* ws, int64_t ws_bytes,
                         void* stream);
int hwgat_stgcn_bn_eval_stats(const float* rm, const float* rv, float eps, float* mean, float* rstd, int C, void* stream);
int hwgat_stgcn_bn_apply(const float* x, const float* mean, const float* rstd, const float* gamma, const float* beta,
                         const float* res, const float* res_mean, const float* res_rstd, const float* res_gamma,
                         const float* res_beta, float* out, int64_t M, int C, int relu, void* stream);
int hwgat_stgcn_bn_bwd(const float* dy, const float* y, const float* x, const float* mean, const float* rstd,
                       const float* gamma, float* dx, float* dgamma, float* dbeta, int64_t M, int C, int train, float* ws,
                       int64_t ws_bytes, void* stream);

/* Graph aggregation over the V <= 32 joints of each of NT frames, Ae = A o E ((3, V, V) each; E NULL = ones).
 * hwgat_stgcn_agg_fwd: out (NT, V, C)[f, w, c] = sum_{k, v} Ae[k, v, w] y[f, v, k C + c], y (NT, V, 3 C).
 * hwgat_stgcn_agg_bwd: dy (NT, V, 3 C) from d = dL/dout, and, when dE is not NULL, dE[k, v, w] = A[k, v, w] sum_{f, c}
 *   y[f, v, k C + c] d[f, w, c] (written; C a multiple of 32; ws >= hwgat_stgcn_agg_bwd_bytes(NT) bytes).
 * hwgat_stgcn_pool_fwd: out (N, C) = mean over the R rows of each clip of x (N, R, C), times the head-dropout factor of
 *   (seed + *seed_base, index n C + c) -- what hwgat_dropout_mask_f32 writes for an (N, C) tensor; p = 0: no dropout.
 * hwgat_stgcn_pool_bwd: dx (N, R, C) = dout[n, c] factor / R.
 * hwgat_stgcn_copy_cols: dst (rows, ld_dst)[r, c] = src (rows, ld_src)[r, c] for c < ld_src, 0 beyond (pads or crops
 *   the channel dimension of the 2- or 3-channel input to a GEMM-able width and back). */
int hwgat_stgcn_agg_fwd(const float* y, const float* A, const float* E, float* out, int64_t NT, int V, int C, void* stream);
int64_t hwgat_stgcn_agg_bwd_bytes(int64_t NT);
int hwgat_stgcn_agg_bwd(const float* y, const float* d, const float* A, const float* E, float* dy, float* dE, int64_t NT,
                        int V, int C, float* ws, int64_t ws_bytes, void* stream);
int hwgat_stgcn_pool_fwd(const float* x, float* out, int N, int R, int C, uint32_t seed, float p,
                         const uint32_t* seed_base, void* stream);
int hwgat_stgcn_pool_bwd(const float* dout, float* dx, int N, int R, int C, uint32_t seed, float p,
                         const uint32_t* seed_base, void* stream);
int hwgat_stgcn_copy_cols(const float* src, int ld_src, float* dst, int ld_dst, int64_t rows, void* stream);

/* ---- DecoupledGCN baseline (ABI 4006; reference hwgat/models/DecoupledGCN.py).  fp32 only, channels-last activations
 * (N, T, V, C) with V <= 32 joints; everything else of a unit (1x1 / temporal convolutions, BatchNorm, pooled head) runs
 * on the hwgat_stgcn_* entry points.  No kernel uses an atomic: every sum has a fixed order.
 *
 * Decoupled aggregation, An (3, G, V, V) the column-normalised learnable adjacency, channel c uses group c mod G
 * (G divides C):
 * hwgat_dgcn_agg_fwd: out (NT, V, C)[f, w, c] = sum_{k, v} An[k, c mod G, v, w] y[f, v, k C + c], y (NT, V, 3 C).
 * hwgat_dgcn_agg_bwd: dy (NT, V, 3 C)[f, v, k C + c] = sum_w An[k, c mod G, v, w] d[f, w, c] and, when dAn is not NULL,
 *   dAn[k, g, v, w] = sum_{f, c = g mod G} y[f, v, k C + c] d[f, w, c] (written; ws >= hwgat_dgcn_agg_bwd_bytes(NT, G)).
 *
 * Attention gates, s_v (N, V), s_t (N, T), s_c (N, C) (any of them NULL = 0):
 * hwgat_dgcn_gate_sum: out = scale * sum over one axis of
 *     h (g' (1 + s_v[n, v]) (1 + s_t[n, t]) (1 + s_c[n, c]) + m[n, t, c] m_scale),   g' = g (N, T, V, C) or 1 when NULL,
 *   the m term absent when m is NULL; axis 0: over t, out (N, V, C); axis 1: over v, out (N, T, C).
 * hwgat_dgcn_gate_apply: out = h (1 + s_v) (1 + s_t) (1 + s_c).
 * hwgat_dgcn_gate_bwd: dh = d (1 + s_v) (1 + s_t) (1 + s_c) + dm1[n, t, c] (1 + s_v) / V + dm0[n, v, c] / T, the gradient
 *   of the gated output and of the two squeezes mean_V h (1 + s_v) (N, T, C) and mean_T h (N, V, C) with respect to h.
 *
 * DropGraph.  z = x, or (x - mean) rstd gamma + beta when mean is not NULL (a BatchNorm read on the fly):
 * hwgat_dgcn_abs_sum: axis 0: out (N, V) = sum_{t, c} |z|; axis 1: out (N, T) = sum_{v, c} |z| fs[n, v] (fs NULL = 1).
 * hwgat_dgcn_draw: out[i] = 1 where the hash uniform of (seed + *seed_base, i) is below p[i], else 0 (p <= 0: never,
 *   p >= 1: always; the uniform of an element does not depend on p).
 * hwgat_dgcn_mask_spatial: mask[n, w] = 0 where sum_v seeds[n, v] A[v, w] > 0.001, else 1; f = mask * scale and
 *   scale[0] = N V / sum(mask) over the whole batch (one workgroup; an all-zero mask gives inf, as the reference).
 * hwgat_dgcn_mask_temporal: mask[n, t] = 1 - max_{|t' - t| <= block / 2} seeds[n, t'] (block odd), f and scale likewise.
 * hwgat_dgcn_merge: out = relu(bn(c) fs1[n, v] ft1[n, t] + r' fs2[n, v] ft2[n, t]), r' = r or its BatchNorm read when
 *   res_mean is not NULL.
 * hwgat_dgcn_merge_bwd: g = dout [out > 0]; dz1 = g fs1 ft1, dz2 = g fs2 ft2.
 * hwgat_dgcn_masked_sum: out = a [ma > 0] + b [mb > 0] (a mask that is NULL passes everything). */
int hwgat_dgcn_agg_fwd(const float* y, const float* An, float* out, int64_t NT, int V, int C, int G, void* stream);
int64_t hwgat_dgcn_agg_bwd_bytes(int64_t NT, int G);
int hwgat_dgcn_agg_bwd(const float* y, const float* d, const float* An, float* dy, float* dAn, int64_t NT, int V, int C,
                       int G, float* ws, int64_t ws_bytes, void* stream);
int hwgat_dgcn_gate_sum(const float* h, const float* g, const float* sv, const float* st, const float* sc, const float* m,
                        float m_scale, float* out, int N, int T, int V, int C, int axis, float scale, void* stream);
int hwgat_dgcn_gate_apply(const float* h, const float* sv, const float* st, const float* sc, float* out, int N, int T,
                          int V, int C, void* stream);
int hwgat_dgcn_gate_bwd(const float* d, const float* sv, const float* st, const float* sc, const float* dm1,
                        const float* dm0, float* dh, int N, int T, int V, int C, void* stream);
int hwgat_dgcn_abs_sum(const float* x, const float* mean, const float* rstd, const float* gamma, const float* beta,
                       const float* fs, float* out, int N, int T, int V, int C, int axis, void* stream);
int hwgat_dgcn_draw(const float* p, float* out, int64_t n, uint32_t seed, const uint32_t* seed_base, void* stream);
int hwgat_dgcn_mask_spatial(const float* seeds, const float* A, float* f, float* scale, int N, int V, void* stream);
int hwgat_dgcn_mask_temporal(const float* seeds, float* f, float* scale, int N, int T, int block, void* stream);
int hwgat_dgcn_merge(const float* c, const float* mean, const float* rstd, const float* gamma, const float* beta,
                     const float* r, const float* res_mean, const float* res_rstd, const float* res_gamma,
                     const float* res_beta, const float* fs1, const float* ft1, const float* fs2, const float* ft2,
                     float* out, int N, int T, int V, int C, void* stream);
int hwgat_dgcn_merge_bwd(const float* dout, const float* out, const float* fs1, const float* ft1, const float* fs2,
                         const float* ft2, float* dz1, float* dz2, int N, int T, int V, int C, void* stream);
int hwgat_dgcn_masked_sum(const float* a, const float* ma, const float* b, const float* mb, float* out, int64_t n,
                          void* stream);

/* ---- smoothed cross-entropy on the logits and device-side evaluation (csrc/loss_eval.hip; reference:
 * hwgat/losses/SmoothCrossEntropy.py, hwgat/utils.py:118-161 evaluate / predictions_plus_true, :324-350 gen_cm_w).
 * logits fp32 (B, C) row-major, target int64 (B); B >= 1 (at most 2^31 - 1) and 1 <= C <= 65536, else HWGAT_ESHAPE.
 * `n_valid` is a DEVICE int32 read when the kernels run (clamped to [0, B]); NULL means all B rows.  Rows at or beyond
 * it are neither read nor written by the forward and the accumulator, and get zeros in the backward.  A target outside
 * [0, C) is never used as an index.  No float atomic: every output is bit-reproducible.
 *
 * hwgat_sce_fwd, per row b with t = target[b] (two launches: the rows, then the mean):
 *   lse[b]      = log sum_j exp(z[b, j]), max-subtracted
 *   row_loss[b] = (1 - eps) (lse - z[b, t]) + eps (lse - mean_j z[b, j]); eps = 0 is plain cross-entropy
 *   rank[b]     = #{j : z[b, j] > z[b, t]} + #{j < t : z[b, j] == z[b, t]}, the target's place in a stable descending sort
 *   pred[b]     = the lowest index that holds the row maximum
 *   loss[0]     = mean of row_loss over the first n_valid rows, summed in a fixed order (n_valid = 0: NaN)
 *   A bad target gives row_loss = NaN (and so the mean) and rank = C; a row with a NaN (or +inf) logit gives lse =
 *   row_loss = NaN, rank = C and pred some index in [0, C).
 * hwgat_sce_bwd: dlogits[b, j] = g[0] / n_valid * (exp(z[b, j] - lse[b]) - (1 - eps) [j == t] - eps / C), g a DEVICE
 *   float (the upstream gradient of the scalar loss); a row with a bad target is NaN throughout.
 *
 * hwgat_eval_accumulate (one workgroup) folds the outputs of one hwgat_sce_fwd into the accumulator block `acc`, which
 * the caller zeroes to reset.  Layout of the block, hwgat_eval_acc_bytes(C, k_max, cap) bytes, offsets in bytes:
 *      0  int64   n_samples                      rows seen (bad targets included)
 *      8  int64   n_batches                      calls with n_valid > 0
 *     16  int64   n_invalid                      rows with a target outside [0, C): counted here and nowhere below
 *     24  double  loss_sum_samples               sum of row_loss
 *     32  double  loss_sum_batches               sum of the batch means loss[0]
 *     40  int64   rank_hist[k_max + 1]           rank_hist[min(rank, k_max)] += 1: top-k hits = sum of the first k entries
 *     ..  int64   confusion[C][C]                confusion[target][pred] += 1
 *     ..  int32   pred_log[cap], target_log[cap] row i of the run at index i while i < cap (cap may be 0); once the log
 *                                                is full, further rows are counted above but not logged */
int hwgat_sce_fwd(const float* logits, const int64_t* target, const int32_t* n_valid, float* lse, float* row_loss,
                  int32_t* rank, int32_t* pred, float* loss, int64_t B, int C, float eps, void* stream);
int hwgat_sce_bwd(const float* logits, const int64_t* target, const int32_t* n_valid, const float* lse, const float* g,
                  float* dlogits, int64_t B, int C, float eps, void* stream);
int64_t hwgat_eval_acc_bytes(int C, int k_max, int64_t cap);
int hwgat_eval_accumulate(void* acc, const float* row_loss, const int32_t* rank, const int32_t* pred,
                          const int64_t* target, const float* loss, const int32_t* n_valid, int64_t B, int C, int k_max,
                          int64_t cap, void* stream);

/* ---- the same loss for one SLICE of a zero-padded batch (train.BatchSlicedCrossEntropyLoss: micro-batches and short
 * batches in one captured train step).  The batch holds *n_rows real rows (a DEVICE int32, read when the kernels run)
 * followed by padding; the slice is its rows [offset, offset + B), `offset` a host integer in [0, 2^31).  The slice's
 * first v = clamp(*n_rows - offset, 0, B) rows are live; logits (B, C), target (B) and the limits on B and C are
 * hwgat_sce_fwd's.  A NULL pointer (n_rows included) or an offset out of range is HWGAT_EINVAL.
 * hwgat_bsce_fwd (three launches: v, the rows, the sums):
 *   live[0]     = v
 *   lse, row_loss, rank, pred: hwgat_sce_fwd's, bit for bit, for the live rows; the other rows are neither read nor written
 *   loss[0]     = sum of row_loss over the live rows, in a fixed order, divided by *n_rows: the slice's share of the
 *                 BATCH mean, so the losses of a batch's slices add up to its mean loss.  v = 0 gives exactly 0, not the
 *                 NaN of an empty mean
 *   correct[0]  = number of live rows with rank 0
 * hwgat_bsce_bwd: dlogits[b, j] = g[0] / *n_rows * (exp(z[b, j] - lse[b]) - (1 - eps) [j == t] - eps / C) for a live row,
 *   exactly 0.0f for every other; a live row with a bad target is NaN throughout.  No float atomic anywhere. */
int hwgat_bsce_fwd(const float* logits, const int64_t* target, const int32_t* n_rows, int64_t offset, float* lse,
                   float* row_loss, int32_t* rank, int32_t* pred, float* loss, int64_t* correct, int32_t* live, int64_t B,
                   int C, float eps, void* stream);
int hwgat_bsce_bwd(const float* logits, const int64_t* target, const int32_t* n_rows, int64_t offset, const float* lse,
                   const float* g, float* dlogits, int64_t B, int C, float eps, void* stream);

/* ---- the slice criterion with two targets and a weight per row (train.MixedCrossEntropyLoss: Mixup / CutMix targets).
 * Arguments, live rows, dead rows, `offset`, the empty slice and bad targets are hwgat_bsce_*'s, word for word; target_b (B)
 * int64 and lam (B) fp32 are slice pointers like target.  With l(t) the row loss hwgat_bsce_fwd computes for target t:
 * hwgat_mbsce_fwd (four launches: v, the rows under target, the rows under target_b, the sums):
 *   row_loss_b, rank_b (B): l(target_b) and target_b's rank of the live rows, hwgat_sce_fwd's bit for bit
 *   row_loss[b] = fadd_rn(fmul_rn(lam, l(t)), fmul_rn(fsub_rn(1, lam), l(t_b))): a row with lam == 1.0f and a finite l(t_b)
 *                 has hwgat_bsce_fwd's bits
 *   rank[b]     = the rank of the DOMINANT label: target's when lam >= 0.5f, else target_b's;  pred, lse: hwgat_sce_fwd's
 *   loss[0], correct[0], live[0]: hwgat_bsce_fwd's sums over row_loss and rank as above, in the same fixed order
 * hwgat_mbsce_bwd: dlogits[b, j] = g[0] / *n_rows * (exp(z[b, j] - lse[b]) - (1 - eps) (lam [j == t] + (1 - lam) [j == t_b])
 *   - eps / C) for a live row, exactly 0.0f for every other; a live row with a bad target or target_b is NaN throughout.
 *   The bracket is formed as fmul_rn(1 - eps, fadd_rn(lam [j == t], fsub_rn(1, lam) [j == t_b])): where t == t_b the column
 *   gets (1 - eps)(lam + (1 - lam)), and that fp32 sum need not be exactly 1 -- such a row may differ from hwgat_bsce_bwd's
 *   in the last bit unless lam is 0 or 1.  A row with lam == 1.0f has hwgat_bsce_bwd's bits.  No float atomic anywhere. */
int hwgat_mbsce_fwd(const float* logits, const int64_t* target, const int64_t* target_b, const float* lam,
                    const int32_t* n_rows, int64_t offset, float* lse, float* row_loss, int32_t* rank, int32_t* pred,
                    float* loss, int64_t* correct, int32_t* live, float* row_loss_b, int32_t* rank_b, int64_t B, int C,
                    float eps, void* stream);
int hwgat_mbsce_bwd(const float* logits, const int64_t* target, const int64_t* target_b, const float* lam,
                    const int32_t* n_rows, int64_t offset, const float* lse, const float* g, float* dlogits, int64_t B,
                    int C, float eps, void* stream);

/* ---- the slice criterion distilled from a teacher (train.DistilledCrossEntropyLoss, train.Distiller): hwgat_mbsce_*'s
 * loss blended with the tempered KL divergence from the teacher's logits.  Arguments, live rows, dead rows, `offset`,
 * *n_rows, the empty slice, bad targets and the limits on B and C are hwgat_bsce_fwd's, word for word; teacher (B, C) fp32
 * is a slice pointer like logits.  target_b and lam may BOTH be NULL: no mixer, every row has the one target (lam = 1) and
 * row_loss_b / rank_b are not touched (they may be NULL then); one NULL and one non-NULL is HWGAT_EINVAL.
 * state: hwgat_kd_state_bytes() = 8 bytes of DEVICE memory, 8-byte aligned: float alpha, tau.  hwgat_kd_set (one thread,
 *   stream-ordered) writes both; alpha outside [0, 1], tau outside [HWGAT_KD_TAU_MIN, HWGAT_KD_TAU_MAX] or a NaN is
 *   HWGAT_ESHAPE before any launch.  The kernels clamp what they read to the same ranges (a NaN: the lower end).
 * For a live row with student logits z, teacher logits u, p = softmax(u / tau), q = softmax(z / tau):
 *   hard        = the row loss hwgat_mbsce_fwd computes (lam NULL: hwgat_bsce_fwd's), bit for bit
 *   lse_s, lse_t (B) fp32 = logsumexp(z / tau), logsumexp(u / tau)
 *   row_kd  (B) fp32 = tau^2 sum_j p_j (log p_j - log q_j); a term with p_j = 0 (u_j = -inf) counts 0.  Evaluated as
 *                 tau^2 (sum_j p_j d_j - log1p(sum_j q_j expm1(d_j))), d_j = (u_j - z_j) / tau - (max u - max z) / tau, the
 *                 sums over j in double: no term of order 1 is cancelled, and a row with u == z bit for bit gives exactly
 *                 0.0f.  A teacher row with a NaN or +inf gives NaN (and so a NaN row_loss and loss); so does a column
 *                 with z_j = -inf and u_j finite, where the divergence is infinite
 *   row_loss    = (1 - alpha) hard + alpha row_kd
 *   t_pred  (B) int32 = the lowest index holding the teacher row's maximum (pred's rule)
 *   lse, rank, pred, correct[0], live[0]: hwgat_mbsce_fwd's
 *   loss[0], kd[0] = the live rows' row_loss, row_kd summed in hwgat_bsce_fwd's fixed order over *n_rows; exactly 0 for an
 *                 empty slice
 *   agree[0]     int64 = live rows with pred == t_pred;  t_correct[0] int64 = live rows whose t_pred is the dominant label
 *   When the alpha word is exactly 0.0f the teacher is not read: row_loss, loss[0] have hwgat_mbsce_fwd's bits (lam NULL:
 *   hwgat_bsce_fwd's), row_kd, lse_s, lse_t and kd[0] are 0, t_pred is -1, agree[0] and t_correct[0] are 0.
 * hwgat_kd_fwd is at most five launches (v, the rows under target_b -- not with lam NULL --, the rows under target, the
 *   rows' KL, the sums): one more than hwgat_mbsce_fwd.
 * hwgat_kd_bwd (one launch): for a live row
 *   dlogits[b, j] = g[0] / *n_rows ((1 - alpha)(exp(z_j - lse) - (1 - eps) hit_j - eps / C)
 *                                   + alpha tau (exp(z_j / tau - lse_s) / Z_s - exp(u_j / tau - lse_t) / Z_t))
 *   with hit_j hwgat_mbsce_bwd's bracket (lam NULL: the one-hot) and Z_s = sum_j exp(z_j / tau - lse_s), Z_t likewise: 1 up
 *   to the rounding of lse_s / lse_t to fp32, summed in double in the fixed order -- the two softmaxes differ by order
 *   1 / tau, and that rounding would otherwise be the gradient's error.  Exactly 0.0f for every dead row.  With the alpha word
 *   exactly 0.0f it evaluates hwgat_mbsce_bwd's expression (lam NULL: hwgat_bsce_bwd's bits) and reads no teacher.
 * No float or double atomic anywhere; a repeat is bit-equal.  Rows off a 16-byte boundary and C % 4 != 0 take the scalar
 * loads; rows of more than 4096 columns are read from memory twice instead of staged. */
#define HWGAT_KD_TAU_MIN 0.25
#define HWGAT_KD_TAU_MAX 32.0
int64_t hwgat_kd_state_bytes(void);
int hwgat_kd_set(void* state, float alpha, float tau, void* stream);
int hwgat_kd_fwd(const float* logits, const float* teacher, const int64_t* target, const int64_t* target_b,
                 const float* lam, const int32_t* n_rows, int64_t offset, const void* state, float* lse, float* row_loss,
                 int32_t* rank, int32_t* pred, float* loss, int64_t* correct, int32_t* live, float* row_loss_b,
                 int32_t* rank_b, float* lse_s, float* lse_t, float* row_kd, int32_t* t_pred, float* kd, int64_t* agree,
                 int64_t* t_correct, int64_t B, int C, float eps, void* stream);
int hwgat_kd_bwd(const float* logits, const float* teacher, const int64_t* target, const int64_t* target_b,
                 const float* lam, const int32_t* n_rows, int64_t offset, const void* state, const float* lse,
                 const float* lse_s, const float* lse_t, const float* g, float* dlogits, int64_t B, int C, float eps,
                 void* stream);

/* ---- the classifier head (csrc/head.hip; reference: the `head` / `classifier` nn.Linear of every model,
 * hwgat/models/HWGATE.py:331,372).  Everything fp32 and row-major; W is (N, K) as nn.Linear stores it.
 *   hwgat_head_fwd:    Y[M, N]  = X[M, K] W^T + bias      (bias may be NULL: no bias)
 *   hwgat_head_bwd_dx: dX[M, K] = dY[M, N] W
 *   hwgat_head_bwd_dw: dW[N, K] = dY^T X,  db[N] = column sums of dY      (db may be NULL: not computed)
 * Shapes: M >= 1 rows (the batch), 1 <= N <= 65536 classes (the range of hwgat_sce_fwd), K % 64 == 0 and 64 <= K <= 1024
 * (every stage width of the models); anything else HWGAT_ESHAPE.  A NULL required pointer, a non-positive M or N, or an
 * X, W, dX or dW that is not 16-byte aligned (those are read and written 16 bytes at a time; Y, dY, bias and db need
 * 4) is HWGAT_EINVAL.  Both are decided before any HIP call.
 * Outputs are overwritten, never accumulated into: nothing needs zeroing, there is no workspace and no state.  Nothing
 * outside [0, M) x [0, N) of Y (and likewise of the other outputs) is written.
 * Exact fp32 on v_mfma_f32_16x16x4_f32, no float atomic.  Each output element is summed in a fixed order that depends
 * only on the length of its reduction (K for Y, N for dX, M for dW and db): row m of Y is a function of X[m, :], W and
 * bias alone and has the same bits in a batch of 64 as in a batch of 1 (dX and dY likewise), and two runs are bit-equal.
 * Non-finite inputs propagate as in the dense product; no part of a product is skipped for what an operand holds. */
int hwgat_head_fwd(const float* X, const float* W, const float* bias, float* Y, int M, int N, int K, void* stream);
int hwgat_head_bwd_dx(const float* dY, const float* W, float* dX, int M, int N, int K, void* stream);
int hwgat_head_bwd_dw(const float* dY, const float* X, float* dW, float* db, int M, int N, int K, void* stream);

/* ---- input modalities (csrc/modality.hip; modality.Modality, the models' `input_modality`).  The four views of a keypoint
 * clip that multi-stream skeleton recognisers train on.  x and out are (B, T, J, C) fp32, contiguous; out must not overlap
 * x (HWGAT_EINVAL).  parent: J int32 words in DEVICE memory, p = parent[j] the joint that joint j hangs on, parent[j] == j a
 * root; the kernel reduces what it reads to [0, J).  parent may be NULL for the kinds that do not read it.
 *   HWGAT_MOD_JOINT        out[b,t,j,c] = x[b,t,j,c]
 *   HWGAT_MOD_BONE         out[b,t,j,c] = x[b,t,j,c] - x[b,t,p,c];  a root gives +0.0 whatever x holds
 *   HWGAT_MOD_MOTION       out[b,t,j,c] = x[b,t+1,j,c] - x[b,t,j,c] for t < T - 1;  0 at t = T - 1
 *   HWGAT_MOD_BONE_MOTION  out[b,t,j,c] = (x[b,t+1,j,c] - x[b,t+1,p,c]) - (x[b,t,j,c] - x[b,t,p,c]), each bracket rounded to
 *                          fp32 (a root's bracket is +0.0), then their difference;  0 at t = T - 1
 * Padding (use_pad != 0): frame (b, t) is padding iff x[b,t,0,0] == pad_value -- hwgat_seq_embed_fwd's rule for the
 * key-padding words.  A padded frame is copied to out unchanged for every kind, and the two motion kinds give 0 at a frame
 * whose successor is padded.  With use_pad == 0 pad_value is not read.
 * Every entry is a copy, one IEEE subtraction or the difference of two: the result is exact.  One launch, one pass, no
 * atomics, no LDS, no workspace.
 * HWGAT_EINVAL: a NULL x or out, a non-positive size, a NULL parent with a bone kind, overlapping x and out.  HWGAT_ESHAPE:
 * kind outside 0..3, J C > 2^20, more than 2^31 - 1 workgroups of 256 entries. */
#define HWGAT_MOD_JOINT 0
#define HWGAT_MOD_BONE 1
#define HWGAT_MOD_MOTION 2
#define HWGAT_MOD_BONE_MOTION 3
int hwgat_modality(const float* x, const int32_t* parent, float* out, int B, int T, int J, int C, int kind, int use_pad,
                   float pad_value, void* stream);

/* ---- score ensemble (csrc/ensemble.hip; ensemble.Ensemble).  z (M, B, C) fp32: the logits of M members; w: M fp32 weights
 * in DEVICE memory, read when the kernel runs (a captured evaluation follows a new weight without a new capture);
 * out (B, C) fp32, overwritten.  1 <= M <= HWGAT_ENS_MAX_MEMBERS and mode 0 or 1, else HWGAT_ESHAPE; a NULL pointer or a
 * non-positive B or C is HWGAT_EINVAL.
 *   HWGAT_ENS_LOGIT  out[b,c] = sum_m w[m] z[m,b,c], every product and sum rounded to fp32, members in order from 0.0: the
 *                    error is at most (M + 1) 2^-24 sum_m |w[m] z[m,b,c]|.  Every member is read.
 *   HWGAT_ENS_PROB   out[b,c] = log sum_m w[m] softmax(z[m,b,:])[c], evaluated as the log-sum-exp over the members of
 *                    log w[m] + z[m,b,c] - lse[m,b] with the largest term taken out: no probability is formed, so none
 *                    underflows.  lse[m,b] = max + log(sum expf(z - max)), the sum and everything after it in double; an
 *                    entry is rounded to fp32 once.  A member whose weight is not > 0 is not read.  With weights summing
 *                    to 1 a row of out is a normalised log-distribution; with one member of weight 1 it is its
 *                    log_softmax.  A class to which every member read gives -inf is -inf.
 * Non-finite logits of a member that is read propagate (a NaN makes its row of out NaN in prob mode, its entry in logit
 * mode); nothing is masked.  One launch, one workgroup per row b, no float atomics, no workspace: a repeat is bit-equal. */
#define HWGAT_ENS_MAX_MEMBERS 8
#define HWGAT_ENS_LOGIT 0
#define HWGAT_ENS_PROB 1
int hwgat_ens_fuse(const float* z, const float* w, float* out, int M, int B, int C, int mode, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HWGAT_HIP_H */
