/*
 * srgpt.h -- C ABI of libsrgpt_hip.so: the MI355X (gfx950) kernels behind SpatialRGPT's region-grounded
 * multimodal forward/generate path.
 *
 * The reference (AnjieCheng/SpatialRGPT @ 2024-12-18) is pure Python; it has no FFI/plugin seam of its
 * own.  Each entry point below therefore names the reference *function* whose
 * arithmetic it replaces (file:line relative to the reference root).  The Python host
 * (spatialrgpt_amd/) keeps the reference's call signatures and binds these symbols with ctypes;
 * INTEGRATION.md shows the stub a reference maintainer would add.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless the name starts with `h_`; tensors are dense row-major
 *   - `dtype` selects the storage type of activations AND weights: SRGPT_F32 or SRGPT_BF16;
 *     accumulation is always fp32.  bf16 is the parity/benchmark dtype, fp32 exists for tight parity
 *     checks of the same code path
 *   - every function only enqueues work on `stream` (a hipStream_t) and returns immediately;
 *     nothing allocates, nothing synchronises (except srgpt_graph_* creation), no globals
 *   - return value: 0 on success, negative SRGPT_ERR_* otherwise; srgpt_last_error() gives the text
 *     (thread-local).  The Python host maps codes to the exceptions the reference raises.
 */
#ifndef SRGPT_H_
#define SRGPT_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* srgpt_stream_t; /* hipStream_t */

enum { SRGPT_F32 = 0, SRGPT_BF16 = 1 };
enum { SRGPT_ACT_NONE = 0, SRGPT_ACT_GELU_ERF = 1, SRGPT_ACT_GELU_TANH = 2, SRGPT_ACT_SILU = 3, SRGPT_ACT_QUICK_GELU = 4 };
enum {
  SRGPT_OK = 0,
  SRGPT_ERR_ARG = -1,      /* -> ValueError */
  SRGPT_ERR_UNSUPPORTED = -2, /* -> NotImplementedError */
  SRGPT_ERR_LAUNCH = -3,   /* -> RuntimeError */
  SRGPT_ERR_STATE = -4     /* -> RuntimeError */
};
/* output-row mapping of srgpt_gemm */
enum {
  SRGPT_OUT_PLAIN = 0,     /* C[m, n]                                                       */
  SRGPT_OUT_DECONV2X = 1   /* ConvTranspose2d(k=2,s=2) pixel shuffle, channels-last (see gemm) */
};

const char* srgpt_last_error(void);
int srgpt_abi_version(void);
/* number of compute units of the current device (host query, used to size persistent grids) */
int srgpt_device_cus(void);

/* ---------------------------------------------------------------------------------------------
 * GEMM family: every nn.Linear / conv-as-GEMM on the path.
 *   C[M,N] = act(A[M,K] @ W[N,K]^T + bias[N]) + residual
 * replaces: HF SiglipAttention/SiglipMLP Linear layers (third-party, called from
 * multimodal_encoder/vision_encoder.py:119-129), region_extractor/base_extractor.py:93-96,125-126
 * (ConvTranspose2d + connectors), multimodal_projector/base_projector.py:76-79,
 * transformers_replace/models/llama/modeling_llama.py:300-336 (q/k/v/o), :194-223 (MLP), :1044 (lm_head).
 *   - A row stride lda, C row stride ldc (elements); W dense [N,K]; K % 8 == 0 (bf16) / K % 4 == 0 (f32)
 *   - bias may be NULL; bias index is n % bias_mod when bias_mod > 0 (deconv: bias per channel)
 *   - residual may be NULL; residual row is (m % res_mod) when res_mod > 0 (position embeddings), ld = N
 *   - out_f32 != 0: C is written as fp32 regardless of dtype (logits.float(), modeling_llama.py:1045)
 *   - out_mode SRGPT_OUT_DECONV2X: A rows are pixels (img, i, j) of a [n_img, gw, gw] grid, N = 4*Cout
 *     ordered n = (a*2+b)*Cout + co; C is the channels-last [n_img, 2gw, 2gw, Cout] map and
 *     element (m,n) lands at pixel (2i+a, 2j+b), channel co.  `gw` passes the grid width.
 *   - ws / ws_bytes: optional fp32 workspace for deterministic split-K (small-M shapes whose tile grid cannot fill
 *     256 CUs: K is cut into <= 8 slabs written to ws and reduced in slab order); NULL disables split-K.
 *     srgpt_gemm_ws_bytes(M, N) is always sufficient.
 * --------------------------------------------------------------------------------------------- */
int64_t srgpt_gemm_ws_bytes(int M, int N);
int srgpt_gemm(const void* A, const void* W, const void* bias, const void* residual, void* C,
               int M, int N, int K, int lda, int ldc, int act, int bias_mod, int res_mod,
               int out_f32, int out_mode, int gw, void* ws, int64_t ws_bytes, int dtype, srgpt_stream_t stream);

/* C[M,N] = A[M,K] @ W[N,K]^T + bias[n] + residual[M,N] and Y[M,N] = norm(C) from one call -- the tail of an attention / MLP block
 * followed by the next block's input norm: LlamaDecoderLayer.forward modeling_llama.py:611-684 (o_proj or down_proj, the residual
 * add, then LlamaRMSNorm :61-75; norm_kind SRGPT_NORM_RMS, bias and norm_b NULL) and the HF SigLIP / CLIP encoder layer (out_proj
 * or fc2 + bias, the residual add, then nn.LayerNorm; SRGPT_NORM_LAYER).  Dense rows (lda = K, ldc = N), no activation.  When the
 * product is split over K the norm rides in the slab reduction (one launch and one pass over the rows less); otherwise it is the
 * srgpt_rmsnorm / srgpt_layernorm launch.  Either way C and Y are bit-identical to srgpt_gemm followed by the norm.  C may alias
 * residual, Y may alias A (not C).  ws as for srgpt_gemm. */
#define SRGPT_NORM_RMS 1
#define SRGPT_NORM_LAYER 2
int srgpt_gemm_norm(const void* A, const void* W, const void* bias, const void* residual, void* C, int M, int N, int K, void* ws,
                    int64_t ws_bytes, int norm_kind, const void* norm_w, const void* norm_b, void* Y, float norm_eps, int dtype,
                    srgpt_stream_t stream);

/* out[M, I] = silu(A @ Wg^T) * (A @ Wu^T) for the stacked weight Wgu = [Wg; Wu] ([2 I, K], the layout srgpt_gemv's swiglu mode
 * reads) -- LlamaMLP's gate / up products and srgpt_silu_mul (below) in one call (modeling_llama.py:194-223).  At 225 .. 272 rows
 * (the bs = 1 prefill) the activation is the epilogue of the product and the [M, 2 I] intermediate is never written; every other
 * shape runs srgpt_gemm into gu_scratch ([M, 2 I], may be NULL only when the fused form applies) and srgpt_silu_mul.  Either way
 * the result is srgpt_gemm + srgpt_silu_mul to the last bit. */
int srgpt_gemm_swiglu(const void* A, const void* Wgu, void* out, int M, int I, int K, void* gu_scratch, void* ws,
                      int64_t ws_bytes, int dtype, srgpt_stream_t stream);

/* qkv[B*T, (Hq + 2 Hkv) D] = A[B*T, K] @ W^T, then RoPE on the q and k heads and the append of k / v to the caches -- the q/k/v
 * projection of a prefill and srgpt_rope_kv_append (below: same arguments, same arithmetic) in one call
 * (LlamaFlashAttention2.forward modeling_llama.py:398-456).  When the product is split over K the rotation rides in the slab
 * reduction; otherwise it is the srgpt_rope_kv_append launch.  Every byte written (qkv, kcache, vcache) is the same either way. */
int srgpt_gemm_rope_kv_append(const void* A, const void* W, void* qkv, int K, void* ws, int64_t ws_bytes, void* kcache,
                              void* vcache, const int* pos0, const void* cos_tab, const void* sin_tab, int B, int T, int Hq,
                              int Hkv, int D, int max_pos, int dtype, srgpt_stream_t stream);

/* GEMM with weight-only fp8 quantisation (the prefill-side companion of srgpt_gemv_w8, BASELINE config 5):
 *   C[M,N] = act( (A[M,K] @ fp8(W8[N,K])^T) * wscale[n] + bias[n] ) + residual[M,N]
 * A / bias / residual / C bf16 (C fp32 if out_f32), W8 = OCP e4m3fn bytes, wscale = one fp32 scale per weight row, fp32
 * accumulation over the fp8 values widened exactly to bf16; with power-of-two scales this equals srgpt_gemm on the dequantised
 * bf16 weights bit for bit.  K % 64 == 0 takes the 256 x 256 MFMA kernel, any other K a scalar fallback.  ws: optional fp32
 * split-K workspace (srgpt_gemm_ws_bytes). */
int srgpt_gemm_w8(const void* A, const void* W8, const float* wscale, const void* bias, const void* residual, void* C,
                  int M, int N, int K, int lda, int ldc, int act, int out_f32, void* ws, int64_t ws_bytes,
                  srgpt_stream_t stream);

/* W8A8 on the fp8 matrix pipe (v_mfma_scale_f32_16x16x128_f8f6f4) -- the opt-in prefill mode of BASELINE configs[4]; the
 * reference has no counterpart (it offers bitsandbytes 8/4-bit loading, llava/model/builder.py:51-60).
 * srgpt_quant_rows_e4m3: x [M, K] bf16 (row stride ldx) -> q [M, K] OCP e4m3fn bytes + scale [M] fp32, per row (token):
 *   scale = the smallest power of two with max|x[m,:]| / scale <= 448, q = e4m3fn(x / scale) round-to-nearest-even (the rule the
 *   weights are quantised with).  K % 8 == 0, 16-byte aligned rows.
 * srgpt_gemm_w8a8: C[M,N] = ( (A8[M,K] @ W8[N,K]^T) * ascale[m] * wscale[n] + bias[n] ) + residual[M,N], fp32 accumulation of
 *   exact e4m3 x e4m3 products, bias / residual / C bf16 (C fp32 if out_f32) with srgpt_gemm's rounding points (the product is
 *   rounded to bf16 before the residual is added): the GEMM of the dequantised operands up to the order of the fp32 sum.  K % 128 == 0, K >= 256, lda % 16 == 0, 16-byte aligned operands; anything else
 *   returns SRGPT_ERR_UNSUPPORTED (no fallback).  ws: optional fp32 split-K workspace (srgpt_gemm_ws_bytes).
 *   Scales: srgpt_quant_rows_e4m3 and the weight quantiser produce POWERS OF TWO, for which scaling commutes exactly with the
 *   fp32 sums; arbitrary fp32 scales are accepted, but the split-K path then scales the per-split slabs by ascale before the
 *   reduction and the un-split path after the whole sum -- results stay deterministic for a given (shape, device, ws_bytes),
 *   yet differ by fp32 roundings between the two paths.  Callers that need path-independent bits pass power-of-two scales. */
int srgpt_quant_rows_e4m3(const void* x, void* q, float* scale, int M, int K, int ldx, srgpt_stream_t stream);
/* ABI 5: the same quantisation with the producer of the rows fused in -- what the W8A8 prefill runs, so the bf16 intermediate is
 * neither written nor read.  Bit-identical to srgpt_rmsnorm / srgpt_silu_mul followed by srgpt_quant_rows_e4m3 (tested); K (inter)
 * up to 16384 columns, else SRGPT_ERR_UNSUPPORTED.
 *   _rmsnorm: rows of LlamaRMSNorm(x; norm_w, eps) (modeling_llama.py:61-75), x [M, K] bf16 with row stride ldx
 *   _swiglu:  rows of silu(gate) * up (LlamaMLP.forward, modeling_llama.py:194-223) of gate_up [M, 2 * inter] = [gate | up] */
int srgpt_quant_rows_e4m3_rmsnorm(const void* x, const void* norm_w, float eps, void* q, float* scale, int M, int K, int ldx,
                                  srgpt_stream_t stream);
int srgpt_quant_rows_e4m3_swiglu(const void* gate_up, void* q, float* scale, int M, int inter, srgpt_stream_t stream);
int srgpt_gemm_w8a8(const void* A8, const float* ascale, const void* W8, const float* wscale, const void* bias,
                    const void* residual, void* C, int M, int N, int K, int lda, int ldc, int out_f32, void* ws,
                    int64_t ws_bytes, srgpt_stream_t stream);

/* Decode-only fused GEMVs (any batch; one bf16 / fp8 row: VALU kernel, 2+ rows: MFMA kernel, 16 rows per weight pass -- all rows of
 * one call on the same kernel), weights streamed once per pass from HBM:
 *   norm_w != NULL : x <- RMSNorm(x) * norm_w first (modeling_llama.py:61-75) (rounded to dtype like torch)
 *   swiglu != 0    : W = [gate rows(N); up rows(N)], out[n] = silu(gate.x) * (up.x) (modeling_llama.py:221)
 *   residual       : out = residual + (W x)   (decoder layer residual adds, modeling_llama.py:650-684)
 * Rounding points (rnd = round to nearest even to dtype; fp32: none), the same in all three kernel files and on every route:
 *   out = rnd(rnd(acc * wscale) + residual) with acc the fp32 sum (wscale: srgpt_gemv_w8 only), swiglu:
 *   out = rnd(rnd(silu(rnd(gate))) * rnd(up)).  out_f32 != 0 stores THAT dtype-rounded value widened to fp32 -- not the unrounded
 *   fp32 sum -- so bf16 logits read back as fp32 equal the bf16 output bit for bit (tests/test_gpu_gemv_exact.py).
 */
int srgpt_gemv(const void* x, const void* W, const void* norm_w, float norm_eps, const void* residual,
               void* out, int batch, int N, int K, int swiglu, int out_f32, int dtype, srgpt_stream_t stream);
/* Same product with weight-only fp8 quantisation (W8A16, BASELINE config 5): W8 = OCP e4m3fn bytes [N (2N if swiglu), K],
 * wscale = one fp32 scale per weight row, x / norm_w / residual / out bf16 (out fp32 if out_f32):
 *   out[b, n] = round_bf16( (sum_k x[b,k] * fp8(W8[n,k])) * wscale[n] ), fp32 accumulation; same fusions as srgpt_gemv.
 * The reference has no fp8 path (it offers bitsandbytes 8/4-bit loading, builder.py:51-60); this replaces the 8-bit option
 * (the 4-bit one: srgpt_gemv_w4 below). */
int srgpt_gemv_w8(const void* x, const void* W8, const float* wscale, const void* norm_w, float norm_eps,
                  const void* residual, void* out, int batch, int N, int K, int swiglu, int out_f32,
                  srgpt_stream_t stream);
/* ABI 8: the two products above with the ROW-STATISTICS HAND-OFF the batched decode step runs on (2+ bf16 rows: the MFMA kernel).
 * LlamaRMSNorm (modeling_llama.py:61-75) needs mean(x^2) of every row of the residual stream; the product that WRITES that row
 * (o_proj / down_proj with the residual add, modeling_llama.py:650-684) has each element in a register, so it publishes per-block
 * partial sums and the product that normalises (q/k/v, gate/up, lm_head) adds them in a fixed order instead of re-reading the
 * rows in every block.  A table is [batch][SRGPT_ROWSS_STRIDE] fp32.
 *   W8 != NULL      : fp8 weights (+ wscale), W ignored; else W bf16
 *   rowss_out       : this product's bf16 output rows get their table written (not with swiglu / out_f32)
 *   rowss_in        : the table of x's rows, published by the call that wrote x (requires norm_w); NULL: computed from x
 * srgpt_gemv_rowss_supported: 1 when (batch, dtype, fp8) takes the kernel that can do this (else call srgpt_gemv / _w8).
 * The statistics' summation order differs from srgpt_gemv's own, so the normalised rows may differ from it by one bf16 ulp;
 * srgpt_llm_decode_step == the composition of THESE entries bit for bit (tests/test_gpu_kernels.py). */
#define SRGPT_ROWSS_STRIDE 512
int srgpt_gemv_rowss_supported(int batch, int dtype, int fp8);
int srgpt_gemv_rowss(const void* x, const void* W, const void* W8, const float* wscale, const void* norm_w, float norm_eps,
                     const void* residual, void* out, int batch, int N, int K, int swiglu, int out_f32, const float* rowss_in,
                     float* rowss_out, int packed_rows, srgpt_stream_t stream);
/* ABI 9: the PACKED decode layout of a streamed matrix.  The MFMA kernel behind srgpt_gemv_rowss multiplies 16 weight rows x 32 k
 * per instruction and wants lane (c = lane & 15, g = lane >> 4) to hold row c, k = 32 s + 8 g .. + 8 of the step.  A row-major
 * matrix delivers that through an LDS transpose per 8-KiB stage; the packed array stores the SAME bytes in operand order, so one
 * coalesced 16-byte load per lane is the fragment (fp8 weights, 8 rows per GPU: the four layer products 56 -> 52 us,
 * profiles/r06_skinny_packed_gr.txt).  Layout, `rows` = 4, 8 or 16 rows per granule, e = bytes per element (1: fp8, 2: bf16),
 * kb = 16 / e ... a k block is 64 k (fp8) or 32 k (bf16):
 *   out[ ((n / rows) * (K / kblock) + k / kblock) * rows * 64  +  ((k % 32) / 8 * rows + n % rows) * 16  +  byte ]
 *   byte = (k % 8) * 2 (bf16)   |   ((k % 64) / 32) * 8 + k % 8 (fp8: the lane's 8 k of two consecutive MFMA steps)
 * N is padded to whole granules with zeros (srgpt_packed_bytes); K %% 64 == 0 (fp8) / K %% 32 == 0 (bf16).  A SwiGLU matrix
 * [gate rows (N); up rows (N)] is packed as ONE matrix of 2 N rows (N %% rows == 0).  srgpt_gemv_rowss takes such an array as
 * W / W8 with packed_rows = rows (0: row-major) and returns bit for bit what it returns for the row-major matrix. */
size_t srgpt_packed_bytes(int N, int K, int elem_bytes, int rows);
int srgpt_pack_decode_weights(const void* W, void* out, int N, int K, int elem_bytes, int rows, srgpt_stream_t stream);
/* Additions under ABI 9: MXFP4 weights (OCP Microscaling FP4), the 4-bit option -- a quarter of the bf16 bytes per streamed matrix.
 * The format of a matrix [N (2 N if swiglu), K], K % 32 == 0:
 *   W4      uint8 [N, K / 2]: element k of a row sits in byte k / 2, the LOW nibble holds even k, the high nibble odd k; a code is
 *           OCP e2m1: bit 3 the sign, bits 2 .. 0 the magnitudes {0, 0.5, 1, 1.5, 2, 3, 4, 6}
 *   wscale8 uint8 [N, K / 32]: one E8M0 byte per 32 consecutive values of a row, value = 2^(byte - 127).  The kernels take bytes
 *           1 .. 254 (the quantiser of the Python host never emits 0 or 255; 255 is NaN in the OCP format and 0 is below the fp32
 *           normal range the conversion instruction reads its scale from): other bytes give unspecified VALUES, never a fault.
 *   value[n, k] = e2m1(code) * 2^(byte - 127), exact in bf16.
 * Opt-in like fp8 and it changes the numbers: every 32 values share one power-of-two scale and have 15 levels.  What that costs in
 * accuracy on a trained checkpoint is UNMEASURED (no checkpoint was available to this project).
 * srgpt_gemv_w4: the decode product over such a matrix, x / norm_w / residual / out bf16 (out fp32 if out_f32):
 *   out[b, n] = round_bf16( sum_k x[b, k] * value[n, k] ), fp32 accumulation of exact products; the fusions and the rounding points
 *   of srgpt_gemv_w8 (above, "Rounding points") without a per-row fp32 scale.  A VALU kernel (v_cvt_scalef32_pk_f32_fp4 applies the
 *   block scale while widening) for 1 .. 4 rows per launch; a longer call is cut into launches of at most 4 rows, each a pass over the
 *   codes, all on this kernel.  K % 32 != 0, a NULL x / W4 / wscale8 / out, or swiglu with residual / out_f32: SRGPT_ERR_ARG.
 * srgpt_dequant_mxfp4: out_bf16 [N, K] row-major = value[n, k] (what the prefill multiplies, and the parity hook). */
int srgpt_gemv_w4(const void* x, const void* W4, const void* wscale8, const void* norm_w, float norm_eps, const void* residual,
                  void* out, int batch, int N, int K, int swiglu, int out_f32, srgpt_stream_t stream);
int srgpt_dequant_mxfp4(const void* W4, const void* wscale8, void* out_bf16, int N, int K, srgpt_stream_t stream);
/* Additions under ABI 9: the prefill-side products over such a matrix (W4A16: bf16 activations and outputs, the ROW-MAJOR codes and
 * scales above; the packed copies below are not involved).  Each takes the arguments of its bf16 counterpart with the operand pair
 * (W4, wscale8) in place of W and a bf16 scratch `expand` [N, K] ([2 I, K] for _swiglu), and returns BIT FOR BIT what the counterpart
 * returns on srgpt_dequant_mxfp4 of the same codes -- C, the norm output Y, the q/k/v buffer and both caches, the SwiGLU output: the
 * product takes the SAME route (kernel family, tile, K splits) as the bf16 call of that (M, N, K, workspace, device), and everything
 * that decides a bit (the k of every MFMA step, the instruction, the accumulators, the K range of a split, the slab order, every
 * epilogue and fused reduction) is the bf16 instance's.  On the direct-to-LDS kernels with K % 64 == 0 the codes are multiplied IN
 * the kernel: the code tile is DMA'd to LDS as bytes and widened between LDS and the MFMA operand (v_cvt_scalef32_pk_bf16_fp4, the
 * block scale as the fp32 `byte << 23`, exact), the dequantised matrix is never written.  Every other route (the whole-M kernel of
 * the 225 .. 272-row prefill, the 256 x 256 tiles of M >= 384, K % 64 != 0) expands the matrix into `expand` first
 * (srgpt_dequant_mxfp4) and runs the bf16 launch on it.  srgpt_gemm_w4_in_kernel (host only; N = I with swiglu) returns 1 if the
 * call of that shape multiplies the codes in the kernel on this device, 0 if it expands: `expand` is written and read only on the
 * expansion path and may be NULL where the answer is 1; otherwise NULL is SRGPT_ERR_ARG before any launch.
 *   srgpt_gemm_w4                C = A W^T + residual                 (srgpt_gemm: no bias / activation, plain rows, C fp32 if out_f32)
 *   srgpt_gemm_w4_norm           the same (dense rows) and Y = RMSNorm(C)        (srgpt_gemm_norm with SRGPT_NORM_RMS, no bias)
 *   srgpt_gemm_w4_swiglu         out = silu(A Wg^T) * (A Wu^T), Wgu4 = [Wg; Wu]  (srgpt_gemm_swiglu)
 *   srgpt_gemm_w4_rope_kv_append q/k/v projection + RoPE + cache append          (srgpt_gemm_rope_kv_append)
 * Scale-byte domain of the equality: 2 .. 252 (as srgpt_gemv_w4p below); other bytes give unspecified values, never a fault; no
 * byte outside the code and scale arrays is read.  SRGPT_ERR_ARG: a NULL A / W4 / wscale8 / output, K % 32 != 0, A or `expand` not
 * 16-byte aligned, codes not 4-byte aligned, and the counterpart's own argument errors.  ws / ws_bytes as for srgpt_gemm. */
int srgpt_gemm_w4(const void* A, const void* W4, const void* wscale8, const void* residual, void* C, int M, int N, int K, int lda,
                  int ldc, int out_f32, void* expand, void* ws, int64_t ws_bytes, srgpt_stream_t stream);
int srgpt_gemm_w4_norm(const void* A, const void* W4, const void* wscale8, const void* residual, void* C, int M, int N, int K,
                       void* expand, void* ws, int64_t ws_bytes, const void* norm_w, void* Y, float norm_eps, srgpt_stream_t stream);
int srgpt_gemm_w4_swiglu(const void* A, const void* Wgu4, const void* wscale8, void* out, int M, int I, int K, void* gu_scratch,
                         void* expand, void* ws, int64_t ws_bytes, srgpt_stream_t stream);
int srgpt_gemm_w4_rope_kv_append(const void* A, const void* W4, const void* wscale8, void* qkv, int K, void* expand, void* ws,
                                 int64_t ws_bytes, void* kcache, void* vcache, const int* pos0, const void* cos_tab,
                                 const void* sin_tab, int B, int T, int Hq, int Hkv, int D, int max_pos, srgpt_stream_t stream);
int srgpt_gemm_w4_in_kernel(int M, int N, int K, int swiglu, int have_ws, int64_t ws_bytes);
/* Addition under ABI 9: W4A8 -- srgpt_gemm_w8a8 (above) with such a matrix as the weight operand, on the block-scaled form of the
 * same instruction (v_mfma_scale_f32_16x16x128_f8f6f4 with B as e2m1): a lane's 32 k of one MFMA are one MX block, so the E8M0 bytes
 * as stored are the instruction's scale operand and the matrix is NOT expanded, on any route and at any M.
 *   C[M,N] = ( (A8[M,K] @ value[N,K]^T) * ascale[m] + bias[n] ) + residual[M,N]
 * A8 / ascale from srgpt_quant_rows_e4m3 (or its fused forms), (W4, wscale8) the ROW-MAJOR codes and scales; bias / residual / C,
 * the rounding points, the route (256 x 256 tiles, deterministic K slabs: srgpt_gemm_w8a8's for that M, N, K, workspace, device) and
 * the remark on power-of-two scales are srgpt_gemm_w8a8's.  Products e4m3 x e2m1 x 2^(byte - 127) are exact; the instruction adds the
 * 128 products of a step in a fixed-width window below the largest one (as under unit scales), so with block scales that differ
 * inside a row's K tile the small blocks lose low bits the fp32 sum of srgpt_gemm_w4 would keep (tests/test_gpu_gemm_w4a8.py states
 * the bound).  Opt-in like W8A8: the activations are quantised, the numbers change.  K % 128 == 0, K >= 256, lda % 16 == 0, A8 and W4
 * 16-byte and wscale8 4-byte aligned; anything else returns SRGPT_ERR_UNSUPPORTED (no fallback), a NULL operand or lda < K / ldc < N
 * SRGPT_ERR_ARG, before any launch.  Scale bytes 1 .. 254; no byte outside the code and scale arrays is read. */
int srgpt_gemm_w4a8(const void* A8, const float* ascale, const void* W4, const void* wscale8, const void* bias, const void* residual,
                    void* C, int M, int N, int K, int lda, int ldc, int out_f32, void* ws, int64_t ws_bytes, srgpt_stream_t stream);
/* Additions under ABI 9: the `_direct` forms of those four (opt-in) -- the whole-M kernel multiplies the codes too.  Each has the
 * signature, the argument errors, the route and the bits of its plain counterpart above (equal to the bf16 counterpart on
 * srgpt_dequant_mxfp4 of the codes, scale-byte domain 2 .. 252; no byte outside the code and scale arrays is read).  They differ in
 * WHERE the codes are expanded: in the kernel wherever the plain entry does so, and also on the whole-M kernel (q/k/v, gate/up and
 * down_proj of a 225 .. 272-row prefill; the fused SwiGLU form included) when K % 64 == 0, there are at least 4 K tiles and the scale
 * bytes of a block's K range (128 rows x 2 bytes per K tile of the block's split) fit the LDS the three stages leave: at most 181
 * K tiles per block.  There the code tile is DMA'd to LDS as bytes (4 KiB instead of 16 per K tile) and the dequantised matrix is
 * neither written nor read.  The 256 x 256 tiles, K % 64 == 32 and a range that does not fit still expand.
 * srgpt_gemm_w4_direct_in_kernel (host only; N = I with swiglu) answers for these entries what srgpt_gemm_w4_in_kernel answers for
 * the plain ones: 1 -- `expand` is neither written nor read and may be NULL; 0 -- the call IS the plain entry's expansion path, and
 * a NULL `expand` is SRGPT_ERR_ARG before any launch. */
int srgpt_gemm_w4_direct(const void* A, const void* W4, const void* wscale8, const void* residual, void* C, int M, int N, int K,
                         int lda, int ldc, int out_f32, void* expand, void* ws, int64_t ws_bytes, srgpt_stream_t stream);
int srgpt_gemm_w4_norm_direct(const void* A, const void* W4, const void* wscale8, const void* residual, void* C, int M, int N, int K,
                              void* expand, void* ws, int64_t ws_bytes, const void* norm_w, void* Y, float norm_eps,
                              srgpt_stream_t stream);
int srgpt_gemm_w4_swiglu_direct(const void* A, const void* Wgu4, const void* wscale8, void* out, int M, int I, int K,
                                void* gu_scratch, void* expand, void* ws, int64_t ws_bytes, srgpt_stream_t stream);
int srgpt_gemm_w4_rope_kv_append_direct(const void* A, const void* W4, const void* wscale8, void* qkv, int K, void* expand, void* ws,
                                        int64_t ws_bytes, void* kcache, void* vcache, const int* pos0, const void* cos_tab,
                                        const void* sin_tab, int B, int T, int Hq, int Hkv, int D, int max_pos,
                                        srgpt_stream_t stream);
int srgpt_gemm_w4_direct_in_kernel(int M, int N, int K, int swiglu, int have_ws, int64_t ws_bytes);
/* Additions under ABI 9: the PACKED MXFP4 decode layout and the MFMA product over it, for 2+ rows per weight pass (W4A16: bf16
 * activations; the codes are widened to bf16 in registers with the block scale applied, v_cvt_scalef32_pk_bf16_fp4, exactly, and fed
 * to the bf16 MFMA of srgpt_gemv_rowss).  srgpt_gemv_w4 stays the format's raw reference; this is an opt-in second copy of a matrix.
 * One array holds the codes AND their E8M0 bytes in granules of SRGPT_MXFP4_GRANULE weight rows; a cell is one granule x 128 k:
 * G * 64 code bytes in MFMA-operand order followed by G * 4 scale bytes (G = SRGPT_MXFP4_GRANULE, a cell = 68 G bytes).  With
 * rows = 2 N if swiglu else N, cell(n, k) = (n / G) * (K / 128) + k / 128:
 *   code of (n, k)        : byte  cell * 68 G + ((k % 32) / 8 * G + n % G) * 16 + (k % 128) / 32 * 4 + (k % 8) / 2, nibble k & 1
 *   scale byte of (n, k)  : byte  cell * 68 G + 64 G + (n % G) * 4 + (k % 128) / 32
 * so ONE coalesced 16-byte load of lane (c = lane & 15, g = lane >> 4) is row c, k = 32 s + 8 g .. + 8 for the four MFMA k steps
 * s = 0 .. 3 of the cell (dword s), and the dword beside the codes holds the four scale bytes of those steps; k is not permuted.
 * Domain: K % 128 == 0, N >= 1; rows past the matrix in its last granule hold code 0 and scale byte 127; with swiglu the N gate
 * rows are followed by the N up rows as ONE matrix of 2 N rows and N % G == 0; anything else is SRGPT_ERR_ARG before any launch
 * (srgpt_mxfp4_packed_bytes: 0).  Size: ceil(rows / G) * (K / 128) * 68 G bytes -- the codes, the scales and the padding.
 * srgpt_unpack_mxfp4 writes W4 / wscale8 back (tests): the round trip is exact.
 * srgpt_gemv_w4p: srgpt_gemv_rowss's contract over such an array (RMSNorm prologue, SwiGLU, residual, fp32 out, rowss_in /
 * rowss_out), any batch >= 1 in passes of 16 rows, all on the MFMA kernel.  With a bf16 W = srgpt_dequant_mxfp4 of the same codes,
 * out equals srgpt_gemv_rowss(x, W, ...) BIT FOR BIT for every fusion and row count (same K split, accumulation and reduction order,
 * same rounding points).  Scale-byte domain of THIS kernel: 2 .. 252 -- every value code * 2^(byte - 127) is then a normal finite
 * bf16 (byte 1 makes 0.5 * 2^-126 a denormal, 253 / 254 overflow bf16 at code 6 / 4); other bytes give unspecified values, never a
 * fault.  Argument errors as srgpt_gemv_rowss; rowss tables need 2 * CUs <= SRGPT_ROWSS_STRIDE (SRGPT_ERR_UNSUPPORTED otherwise).
 * The binding table (the rules of srgpt_pack13_bind): srgpt_mxfp4_bind(W4, packed, N, K, swiglu) records on the host that the code
 * array at address W4 has this packed copy; process-global, mutex-protected, keyed by the address, a lookup matches only the exact
 * (N, K, swiglu); a second bind replaces the first; srgpt_mxfp4_unbind returns 1 if there was a binding and must be called BEFORE
 * either buffer is freed; srgpt_mxfp4_bound: 1 / 0.  Every decode-shaped step of an MXFP4 engine (plain, batched, lookup, their
 * graphs) looks wqkv4[i], wo4[i], wgu4[i], wdown4[i] up at launch / capture time: with 2+ rows and ALL of them bound with their
 * shapes the layer products run srgpt_gemv_w4p with the row-statistics hand-off and lm_head srgpt_gemv_rowss; otherwise (one row, or
 * any matrix unbound) every launch is srgpt_gemv_w4's, as without bindings. */
#define SRGPT_MXFP4_GRANULE 16
size_t srgpt_mxfp4_packed_bytes(int N, int K, int swiglu);
int srgpt_pack_mxfp4(const void* W4, const void* wscale8, void* packed, int N, int K, int swiglu, srgpt_stream_t stream);
int srgpt_unpack_mxfp4(const void* packed, void* W4, void* wscale8, int N, int K, int swiglu, srgpt_stream_t stream);
int srgpt_gemv_w4p(const void* x, const void* packed, const void* norm_w, float norm_eps, const void* residual, void* out, int batch,
                   int N, int K, int swiglu, int out_f32, const float* rowss_in, float* rowss_out, srgpt_stream_t stream);
int srgpt_mxfp4_bind(const void* W4, const void* packed, int N, int K, int swiglu);
int srgpt_mxfp4_unbind(const void* W4);
int srgpt_mxfp4_bound(const void* W4);
/* Additions under ABI 9: the WIDE weight pass of the MFMA decode products -- 17 to 32 rows against ONE stream of the weights (opt-in).
 * srgpt_gemv_rowss and srgpt_gemv_w4p cut a call into passes of 16 rows, the M side of one v_mfma_f32_16x16x32_bf16, and every pass
 * reads the whole matrix; a wide pass carries a chunk of 17 - 32 rows as two 16-row M tiles that share each weight fragment.
 * srgpt_gemv_rowss_wide / srgpt_gemv_w4p_wide: the arguments, argument errors and fusions of the 16-row forms.  A call is cut into
 * chunks of 32 rows and a tail; a tail of 16 rows or fewer runs the 16-row form's launch for its row count (40 rows = 32 + 8), and a
 * call of 16 rows or fewer IS the 16-row form.  Row r of a wide chunk has, bit for bit, the output (and the published statistics) of a
 * 16-row pass that holds it: the column split, a wave's K range, the k order, one accumulator per weight tile and M tile, the
 * wave-ordered reduction and the epilogues do not depend on the row count.  (The 16-row forms on a call of 17 - 31 rows end with a
 * pass of FEWER than 9 rows, which sums even and odd k steps on two accumulators: those rows differ from the wide entry's in the
 * last bits -- the reason the option is off by default.)  A product whose wide instance is not built or does not pay keeps passes of 16:
 * srgpt_gemv_wide_pass_rows(batch, fp8, packed, w4, N, K, norm, swiglu) returns the rows per pass the wide entries take for such a call
 * (bf16 activations; packed: rows per granule, 0 row-major; w4: packed MXFP4) -- 32, or 16. */
int srgpt_gemv_rowss_wide(const void* x, const void* W, const void* W8, const float* wscale, const void* norm_w, float norm_eps,
                          const void* residual, void* out, int batch, int N, int K, int swiglu, int out_f32, const float* rowss_in,
                          float* rowss_out, int packed_rows, srgpt_stream_t stream);
int srgpt_gemv_w4p_wide(const void* x, const void* packed, const void* norm_w, float norm_eps, const void* residual, void* out, int batch,
                        int N, int K, int swiglu, int out_f32, const float* rowss_in, float* rowss_out, srgpt_stream_t stream);
int srgpt_gemv_wide_pass_rows(int batch, int fp8, int packed, int w4, int N, int K, int norm, int swiglu);
/* Additions under ABI 9: bf16 weights as LOSSLESS 13-bit codes for the batch-1 decode step -- 0.8125 of the bytes per streamed
 * matrix and bit for bit the results of srgpt_gemv.  Not a quantisation: a bf16 weight is s | e8 | m7, the exponents of a weight row
 * lie within a few dozen values below the row's largest, so a row stores an even base exponent b = max(emax - 31, 1) rounded up to
 * even, and each weight s | c5 | m7 with c = e - b in [0, 31].  A row holding a weight that does not fit -- exponent field 0 (zero,
 * denormal), 255 (Inf, NaN), or below b -- is an EXCEPTION ROW: flagged, and read from the raw matrix instead, so every bf16 matrix
 * round-trips exactly.  The matrix [N, K] row-major bf16, K % 512 == 0 (a SwiGLU matrix: its 2 N rows as one matrix):
 *   packed  srgpt_pack13_bytes(N, K, &flag_bytes) bytes: per row ceil(K / 2048) groups of 3328 bytes (K = 4096: 6656 per row against
 *           8192); a group holds 4 x 64 x 8 weights as a plane of sign bits (256 B), of c >> 1 nibbles (1 KiB) and of low bytes
 *           e0 | m7 (2 KiB), each ordered [lane][bytes] so that a wave loads it with one instruction and lane l receives the
 *           weights k = ((4 g + t) * 64 + l) * 8 + i of the raw kernel's loads (csrc/pack13.h has the bit positions)
 *   flags   flag_bytes bytes: one 32-bit word per row -- b / 2 replicated into its four bytes, or 0xffffffff for an exception row
 *           -- and one more word, the number of exception rows
 * srgpt_pack13 runs on the device, synchronises the stream and returns the number of exception rows (>= 0) or an error (< 0);
 * srgpt_unpack13 writes the exact bf16 matrix back (coded rows from the planes, exception rows from W_raw): tests and debugging.
 * srgpt_gemv_p13: srgpt_gemv's product for ONE bf16 row of x over such a copy, same fusions (RMSNorm prologue, SwiGLU, residual,
 * fp32 out) and the same bits: per row the same fp32 accumulation order, reduction and rounding points; exception rows are streamed
 * from W_raw, which must be the matrix the copy was packed from.
 * The binding table: srgpt_llm_weights has no field for these copies; srgpt_pack13_bind(W_raw, packed, flags, N, K) records, on the
 * host, that the raw matrix at address W_raw has this packed copy.  srgpt_llm_decode_step (and its _ex / _proc / graph forms), in a
 * bf16 engine without fp8 / MXFP4 copies and with ONE row per step, looks up wqkv[i], wgu[i] (2 inter rows), wdown[i] and lm_head
 * at launch / capture time and streams the packed copy of each matrix bound with exactly its shape; everything else -- 2+ rows,
 * lookup steps, prefill, srgpt_gemv itself -- reads the raw matrices.  Unbind (srgpt_pack13_unbind: 1 if there was a binding)
 * BEFORE the raw or the packed buffer is freed or overwritten; a graph captured while bound keeps reading the packed copy.
 * srgpt_pack13_bound: 1 / 0.  The table is mutex-protected and GLOBAL TO THE PROCESS, one binding per raw address: a second bind of
 * an address replaces the first, and an unbind removes whichever is there -- two owners of one raw matrix (two engines over the
 * same device tensors) must not both bind it; check srgpt_pack13_bound first, or bind a matrix of your own (the Python loader
 * clones a shared matrix before it binds).  o_proj (wo[i]) is never looked up: the attention launch prefetches its raw bytes. */
size_t srgpt_pack13_bytes(int N, int K, size_t* flag_bytes);
int srgpt_pack13(const void* W, int N, int K, void* packed, void* flags, srgpt_stream_t stream);
int srgpt_unpack13(const void* packed, const void* flags, const void* W_raw, int N, int K, void* out, srgpt_stream_t stream);
int srgpt_gemv_p13(const void* x, const void* packed, const void* flags, const void* W_raw, const void* norm_w, float norm_eps,
                   const void* residual, void* out, int N, int K, int swiglu, int out_f32, srgpt_stream_t stream);
int srgpt_pack13_bind(const void* W_raw, const void* packed, const void* flags, int N, int K);
int srgpt_pack13_unbind(const void* W_raw);
int srgpt_pack13_bound(const void* W_raw);

/* ---------------------------------------------------------------------------------------------
 * Normalisations.
 * srgpt_layernorm: nn.LayerNorm over the last dim (+ optional activation) -- HF SigLIP layer_norm1/2,
 *   base_projector.py:75 LayerNorm(4C), and LayerNorm2d over channels of a channels-last map followed by
 *   GELU (base_extractor.py:12-24,94-95).
 * srgpt_rmsnorm: LlamaRMSNorm (modeling_llama.py:61-75).
 * --------------------------------------------------------------------------------------------- */
int srgpt_layernorm(const void* x, const void* w, const void* b, void* y, int rows, int cols, float eps,
                    int act, int dtype, srgpt_stream_t stream);
int srgpt_rmsnorm(const void* x, const void* w, void* y, int rows, int cols, float eps, int dtype,
                  srgpt_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Attention.
 * srgpt_attention: softmax(scale * Q K^T [+ causal]) V with fp32 softmax, GQA by head index division.
 *   replaces HF SiglipAttention eager/sdpa (non-causal, called via vision_encoder.py:119-129) and
 *   LlamaFlashAttention2 / flash_attn_func (modeling_llama.py:398-566) for prefill.
 *   Q[b, t, h, :]  at q  + b*q_bs  + t*q_ts  + h*q_hs ; K/V[b, s, hk, :] likewise; O dense [b, t, h, d].
 *   causal: key s visible to query t iff s <= t + (Tk - Tq).
 *   kv_len (device int[B], may be NULL): per-row number of valid keys (right-padded batches).
 *   A query with no visible key (kv_len[b] = 0, or causal with t + (Tk - Tq) < 0) yields zeros.
 * --------------------------------------------------------------------------------------------- */
int srgpt_attention(const void* q, const void* k, const void* v, void* o, int B, int Tq, int Tk, int Hq,
                    int Hkv, int D, int64_t q_bs, int64_t q_ts, int64_t q_hs, int64_t k_bs, int64_t k_ts,
                    int64_t k_hs, int64_t v_bs, int64_t v_ts, int64_t v_hs, float scale, int causal,
                    const int* kv_len, int dtype, srgpt_stream_t stream);

/* srgpt_attention_append: causal attention of NEW query rows over a LIVE cache, every row at a position of its own -- HF's cached
 *   forward (modeling_llama.py:398-456: key_states / value_states grown by past_key_value, the queries of the new positions only;
 *   llava_arch.py:355-385 is the caller's side of it) for a multi-token segment.
 *   Query t of row b sits at absolute position q_pos0[b] + t (q_pos0: device int[B]); key s is visible to it iff
 *   s <= q_pos0[b] + t and s < min(kv_len[b], Tk) (kv_len NULL: Tk).  Tk is the HOST's upper bound on the keys any row may see: it
 *   sizes the tile loop and the kernel selection, which is srgpt_attention's, unchanged.  Shapes, strides and both kernel families as
 *   for srgpt_attention; q_pos0 = NULL is SRGPT_ERR_ARG (that case is srgpt_attention).  With q_pos0[b] = Tk - Tq for every row the
 *   output equals srgpt_attention(causal = 1) bit for bit.  A query with no visible key yields zeros; the output rows of padded
 *   queries (t beyond the row's segment) are unspecified but stay inside o[B, Tq, Hq, D]. */
int srgpt_attention_append(const void* q, const void* k, const void* v, void* o, int B, int Tq, int Tk, int Hq, int Hkv, int D,
                           int64_t q_bs, int64_t q_ts, int64_t q_hs, int64_t k_bs, int64_t k_ts, int64_t k_hs, int64_t v_bs,
                           int64_t v_ts, int64_t v_hs, float scale, const int* q_pos0, const int* kv_len, int dtype,
                           srgpt_stream_t stream);

/* RoPE + KV-cache append (modeling_llama.py:81-191 rotary, :451-456 cache growth -- here a static cache).
 *   qkv: [B*T, (Hq+2Hkv)*D] packed projections; q is rotated in place; rotated k and v are written to
 *   kcache/vcache [B, Hkv, max_pos, D] at positions pos0[b] + t  (pos0: device int[B], NULL = 0).
 *   cos_tab/sin_tab: [max_pos, D/2] in `dtype`, built ONCE at load time by the host exactly as
 *   LlamaRotaryEmbedding does (fp32 angle = position * inv_freq, cos/sin, cast to dtype; linear
 *   scaling of language_model/builder.py:31-38 folded into inv_freq) -- a table, not on-device trig. */
int srgpt_rope_kv_append(void* qkv, void* kcache, void* vcache, const int* pos0, const void* cos_tab,
                         const void* sin_tab, int B, int T, int Hq, int Hkv, int D, int max_pos, int dtype,
                         srgpt_stream_t stream);

/* Decode attention for one new token per sequence against the static cache, fused with RoPE of the new
 * q/k and the cache append (same reference lines as above + flash-attn decode, modeling_llama.py:540-566).
 *   qkv [B, (Hq+2Hkv)*D] raw projections of the new token; pos (device int[B]) = tokens already cached.
 *   ws: fp32 workspace of srgpt_decode_attn_ws_floats(B,Hq,D) floats: per-split partials followed by one arrival ticket per
 *   (sequence, kv head).  The tickets must be ZERO before the first launch (zero the workspace once when it is allocated);
 *   every launch leaves them zero again.  One kernel: the split that arrives last merges the partials.  out [B, Hq*D].
 *   The key ranges of the splits depend on pos only -- for caches of up to 4096 positions (2048 from two sequences up on the VALU
 *   kernel) the output bits do NOT depend on max_pos (a pooled cache may be larger than the request needs); larger caches change
 *   the split count.  bf16 with D = 128 runs on the matrix pipe (fixed 64-key ranges), everything else on the VALU kernel. */
int64_t srgpt_decode_attn_ws_floats(int B, int Hq, int D);
int srgpt_decode_attention(const void* qkv, void* kcache, void* vcache, const int* pos, const void* cos_tab,
                           const void* sin_tab, void* out, float* ws, int B, int Hq, int Hkv, int D,
                           int max_pos, int dtype, srgpt_stream_t stream);
/* Additions under ABI 9: decode attention for T NEW TOKENS per sequence in one launch -- the next token and T - 1 drafted ones of
 * prompt-lookup decoding (HF generate(prompt_lookup_num_tokens = T - 1); the model side is the cached forward over input_ids
 * [1, T], modeling_llama.py:398-456).  Token t of sequence b sits at position pos[b] + t and sees the keys s <= pos[b] + t.
 *   qkv [B, T, (Hq+2Hkv)*D] raw projections; out [B, T, Hq*D]; pos, caches and tables as for srgpt_decode_attention.  The T new k / v
 *   rows are roped and appended at pos[b] .. pos[b] + T - 1; pos itself is NOT advanced (the caller decides how many rows it keeps).
 *   bf16 with D = 128 runs on the matrix pipe, query head g of token t in column t * G + g of the 16 the single-token kernel leaves
 *   mostly empty (G = Hq / Hkv): T * G <= 16, else SRGPT_ERR_UNSUPPORTED before any launch.  qkv is only read.  Output row t EQUALS,
 *   bit for bit, what srgpt_decode_attention returns for token t's projections at position pos[b] + t over a cache that holds the
 *   rows before it, and so do the appended cache rows; the bits do not depend on max_pos up to 4096.
 *   Every other dtype / head_dim (the fp32 parity path) is a composition: one RoPE / append launch, which ROTATES THE q HEADS OF
 *   qkv IN PLACE like srgpt_rope_kv_append, then srgpt_attention_append's one-wave kernel with q_pos0 = pos and Tk = max_pos (it
 *   reads no key behind a row's own position, whatever the cache holds there).  Slow, correct.
 *   A token with pos[b] + t >= max_pos (or pos[b] outside 0 .. max_pos - 1) is neither appended nor attended: its output row is
 *   unspecified but inside out, and no byte outside the caches is written whatever pos holds.
 *   ws: srgpt_decode_attn_multi_ws_floats(B, T, Hq, D) floats -- B * T * Hq * 64 partial rows of D + 2 floats, then B * Hq arrival
 *   tickets, which must be ZERO before the first launch; every launch leaves them zero again. */
int64_t srgpt_decode_attn_multi_ws_floats(int B, int T, int Hq, int D);
int srgpt_decode_attention_multi(void* qkv, void* kcache, void* vcache, const int* pos, const void* cos_tab,
                                 const void* sin_tab, void* out, float* ws, int B, int T, int Hq, int Hkv, int D,
                                 int max_pos, int dtype, srgpt_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Region extractor (SpatialRGPT specific).
 * srgpt_region_pool: MaskPooling.forward (region_extractor/base_extractor.py:32-84) for ONE image:
 *   bilinear resample (align_corners=False, no antialias, scale_factor semantics of F.interpolate) of the
 *   M masks [M, mh, mw] (dtype) to the fw x fw feature grid, cast to dtype, L1-normalise
 *   (sum + 1e-8), weighted reduce over feat [fw*fw, C] -> out [M, C].  Rounding points follow SURVEY 9.2.
 *   rscale_h/w = (float)(1.0 / scale_factor) as ATen's upsample kernel receives it (host computes
 *   scale_factor = sqrt(L / (mh*mw)) in double like base_extractor.py:53-54); M <= 16 per call.
 *   mask_dtype: storage type of `masks` (SRGPT_F32 or SRGPT_BF16) -- the reference does mask.float().
 *   ws: fp32 workspace of srgpt_region_pool_ws_floats(M, fw, C) floats (resampled masks, per-slab sums and partials, arrival
 *   tickets -- it need not be initialised: the first of the two launches re-arms the tickets).  Two launches, no float atomics:
 *   every sum runs in a fixed order, so the result does not depend on scheduling.
 * srgpt_avgpool: AdaptiveAvgPool2d(out_w) on a channels-last map (base_extractor.py:123,145).
 * srgpt_s2d: DownSampleBlock (multimodal_projector/base_projector.py:32-52) -- zero-pad to even, 2x2
 *   space-to-depth in the reference's (column-major block) order; [n, g*g, C] -> [n, ceil(g/2)^2, 4C].
 * srgpt_im2col: patch extraction for the SigLIP patch-embed conv (Conv2d k=s=patch, 'valid'):
 *   images [n,3,S,S] -> [n*g*g, kp] rows ordered (c, ky, kx), zero-padded from 3*p*p to kp columns.
 * --------------------------------------------------------------------------------------------- */
int64_t srgpt_region_pool_ws_floats(int M, int fw, int C);
int srgpt_region_pool(const void* feat, const void* masks, void* out, float* ws, int M, int mh, int mw,
                      int fw, int C, float rscale_h, float rscale_w, int mask_dtype, int dtype,
                      srgpt_stream_t stream);
/* The same pooling straight from the caller's RAW uint8 masks [M, rh, rw]: ys[mh] / xs[mw] (device int32) are the
 * cv2.INTER_NEAREST source row / column of every row / column of the mh x mw processor-size mask the reference builds on the host
 * (mm_utils.py:477-532); the kernel's bilinear taps read through them, so nearest resize, float(uint8) and the resample are one
 * pass over the raw bytes.  Bit-identical to srgpt_mask_resize_nearest followed by srgpt_region_pool. */
int srgpt_region_pool_u8(const void* feat, const void* masks_u8, const int* ys, const int* xs, void* out, float* ws, int M,
                         int rh, int rw, int mh, int mw, int fw, int C, float rscale_h, float rscale_w, int dtype,
                         srgpt_stream_t stream);
int srgpt_avgpool(const void* x, void* y, int n_img, int in_w, int out_w, int C, int dtype,
                  srgpt_stream_t stream);
int srgpt_s2d(const void* x, void* y, int n_img, int g, int C, int dtype, srgpt_stream_t stream);
int srgpt_im2col(const void* images, void* out, int n_img, int S, int patch, int kp, int dtype,
                 srgpt_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Token stream (llava/model/llava_arch.py:434-539).
 * srgpt_embed_rows: out[i,:] = table[ids[i],:]   (embed_tokens; ids are int64, -200 already mapped to 0)
 * srgpt_scatter_rows: dst[idx[i],:] = src[src_idx ? src_idx[i] : i,:]  (image / <mask> / <depth> row
 *   placement; int32 indices; idx[i] < 0 skips the row)
 * srgpt_silu_mul: out = silu(gate) * up over [rows, inter] from a packed [rows, 2*inter] buffer
 * srgpt_argmax: ids_out[b] = argmax_v logits[b, v] (fp32 logits; first max wins like torch.argmax)
 * --------------------------------------------------------------------------------------------- */
int srgpt_embed_rows(const void* table, const int64_t* ids, void* out, int n, int cols, int dtype,
                     srgpt_stream_t stream);
/* ABI 8: the whole splice of prepare_inputs_labels_for_multimodal (llava_arch.py:420-611) on the device, ids never leave it.
 * srgpt_splice_plan (one block per prompt): from ids [B, P] int64 (+ optional attention mask [B, P] bytes) builds, per prompt, the
 *   source of every output row -- desc [B][Tcap][2] = {kind | src << 2, prompt position or -1}; kind 0: embedding row `src` (a text
 *   id), 1: image_features row, 2: mask-embedding row, 3: depth-embedding row -- following the reference rule by rule: masked-out
 *   positions dropped (:434-447), each -200 sentinel replaced by the nimg_feat rows of the NEXT image over the batch (:453-469,
 *   :506-511), the <mask> / <depth> ids of a prompt that owns images replaced IN ORDER by the region embeddings of the prompt's first
 *   image (:470-505; img_info[i] = {rows of image i's region embeddings or -1 if it has none, their first row in the concatenated
 *   embedding matrix}), the prompt cut at max_len (> 0; :541-547).  stats [B][SRGPT_SPLICE_STATS] ints = {length, length before the
 *   cut, sentinels, <mask> ids, <depth> ids, first image index, min / max id sent to the embedding table}: what the host reads back
 *   (the batch's T = max length, and the reference's error / warning conditions).  Tcap >= P + n_images_total * (nimg_feat - 1).
 *   scratch: srgpt_splice_scratch_ints(B, n_images_total) ints.
 * srgpt_splice_gather (one block per output row): out [B, T, cols] = the described rows, prompts shorter than T padded with zero
 *   rows on the right (left_pad: on the left, :549-611); labels_out [B, T] (optional) = labels [B, P] at the row's prompt position,
 *   ignore_index on image rows and padding; attn_mask_out [B, T] bytes (optional) = 1 on real rows. */
#define SRGPT_SPLICE_STATS 8
int64_t srgpt_splice_scratch_ints(int B, int n_images_total);
int srgpt_splice_plan(const int64_t* ids, const unsigned char* attn_mask, int B, int P, int nimg_feat, int n_images_total,
                      const int* img_info, int use_masks, int use_depths, int64_t mask_id, int64_t depth_id, int max_len, int Tcap,
                      int* desc, int* stats, int* scratch, srgpt_stream_t stream);
int srgpt_splice_gather(const int* desc, const int* stats, int B, int Tcap, int T, int left_pad, int cols, int dtype,
                        const void* embed, const void* image_features, const void* mask_embeds, const void* depth_embeds,
                        const int64_t* labels, int P, int64_t ignore_index, void* out, int64_t* labels_out,
                        unsigned char* attn_mask_out, srgpt_stream_t stream);
/* Additions under ABI 9: prefix reuse across requests -- how much of the last request is the head of this one.  Both only enqueue
 * work (nothing allocates, nothing synchronises) and write ONE int; argument errors (a NULL pointer, a negative count, row_bytes < 1)
 * are SRGPT_ERR_ARG before any launch.  The results are minima over "first row that differs": they do not depend on scheduling,
 * and out[] needs no initial value.
 * srgpt_rows_match: a, b = [rows, row_bytes] bytes, any alignment; out[0] = the number of LEADING rows of a that equal the same rows
 *   of b byte for byte, 0 .. rows (-0.0 differs from 0.0, equal NaN bytes are equal; no hashing, so no false hit).  rows = 0: 0.
 * srgpt_splice_match (one prompt): desc_new [len_new][2], desc_old [n_old_rows][2] as srgpt_splice_plan leaves a prompt's rows; only
 *   the first int of a row (kind | src << 2) is compared.  The OLD sequence is desc_old's rows followed by n_gen_old rows of kind 0
 *   whose src are the ids gen_old[j] (int64: the ids the earlier request generated).  out[0] = the number of leading rows
 *   r < min(len_new, n_old_rows + n_gen_old) whose keys are equal; a row of kind 2 or 3 (mask / depth embedding) with
 *   src >= n_regions_common counts as different.  Every length may be 0; the pointers must not be NULL even then. */
int srgpt_rows_match(const void* a, const void* b, int rows, int64_t row_bytes, int* out, srgpt_stream_t stream);
int srgpt_splice_match(const int* desc_new, int len_new, const int* desc_old, int n_old_rows, const int64_t* gen_old, int n_gen_old,
                       int n_regions_common, int* out, srgpt_stream_t stream);
/* ABI 9: beam search's cache permutation on the device (HF `_reorder_cache`): kcache / vcache [layers, batch * num_beams, kv_heads,
 * max_pos, head_dim]; row r of the first `live` positions of every layer := row beam_idx[r] (int64, device; an index never leaves
 * its batch item's num_beams rows).  In place, one launch; 2 ... 8 beams (else SRGPT_ERR_UNSUPPORTED: permute on the caller's side). */
int srgpt_kv_beam_reorder(void* kcache, void* vcache, const int64_t* beam_idx, int layers, int batch, int num_beams, int kv_heads,
                          int max_pos, int head_dim, int live, int dtype, srgpt_stream_t stream);
int srgpt_scatter_rows(const void* src, const int* src_idx, const int* idx, void* dst, int n, int cols,
                       int dtype, srgpt_stream_t stream);
int srgpt_silu_mul(const void* gu, void* out, int rows, int inter, int dtype, srgpt_stream_t stream);
int srgpt_argmax(const float* logits, int64_t* ids_out, int B, int V, srgpt_stream_t stream);
/* Causal-LM loss of LlamaForCausalLM.forward(labels=...) (modeling_llama.py:1047-1058) over already SHIFTED operands:
 * logits fp32 [rows, V] (positions 0..T-2 of every sequence), labels int64 [rows] (positions 1..T-1); rows whose label is
 * ignore_index (-100) do not count.  row_loss: scratch [rows] fp32; out[0] = mean loss (nan if no target), out[1] = targets. */
int srgpt_cross_entropy(const float* logits, const int64_t* labels, float* row_loss, float* out, int rows, int V,
                        int64_t ignore_index, srgpt_stream_t stream);


/* Sampling parameters of the decode step (ABI 6): a block in DEVICE memory, read by the kernels of every step -- one captured graph
 * serves every setting; the host rewrites the block between requests (hipMemcpyAsync on the decode stream).  The warper chain is
 * HF GenerationMixin.sample's, as the reference's interactive callers reach it (demo/gradio_web_server_multi.py:202-213,
 * llava/eval/model_vqa.py:66-80): scores = logits / temperature -> TopKLogitsWarper (everything below the k-th largest score is
 * removed, ties at it kept) -> TopPLogitsWarper (ascending cumulative softmax; entries whose cumulative mass is <= 1 - top_p are
 * removed, never the largest) -> one categorical draw from the softmax of what is left.
 *   Two samplers read this block.  SRGPT_SAMPLER_TOPK64 (srgpt_sample, the decode step's default): top_k 1 .. 64 with any top_p;
 *   top_k = 0: no top-k filter -- then top_p must be >= 1 (pure temperature sampling, drawn by Gumbel-max over the whole
 *   vocabulary).  SRGPT_SAMPLER_FULL (ABI 9 additions: srgpt_sample_full and the _ex entry points): EVERY setting -- top_k 0 (off)
 *   or 1 .. any (clamped to the vocabulary), top_p in [0, 1] -- over the whole vocabulary (V <= 262144).
 *   Randomness: Philox4x32-10, key = seed, counter = (counter, sequence, ...); every step advances `counter` by one. */
typedef struct {
  float temperature;   /* > 0 */
  int top_k;
  float top_p;         /* (0, 1]; >= 1 switches the top-p filter off */
  float top_p_rm;      /* (float)(1.0 - (double)top_p): the removal threshold exactly as HF's comparison sees it */
  uint64_t seed;
  uint64_t counter;
  int* kept_out;       /* parity hook (device, may be NULL): int[batch][257] = the kept-set size, then its token ids best first
                        * (srgpt_sample_rows, srgpt_sample_seq_rows and the sampled lookup steps: int[rows][257]) */
} srgpt_sampling;

/* Stand-alone draw over fp32 logits [B, V] with the parameter block above (what the decode step runs after its lm_head):
 * tok_out[b] = the drawn id; advances sp->counter.  ws = srgpt_sample_ws_bytes(B) bytes of scratch.  V <= 262144. */
int64_t srgpt_sample_ws_bytes(int B);
int srgpt_sample(const float* logits, srgpt_sampling* sp, int64_t* tok_out, void* ws, int B, int V, srgpt_stream_t stream);
/* ABI 8: the parameter block lives on the device, so settings outside the served range (top_k > 64; top_p < 1 with top_k = 0) cannot
 * be refused at the call: the kernels raise a bit in the workspace's error word instead of drawing from a silently clamped
 * distribution.  srgpt_sample CLEARS that word when it starts, so srgpt_sample_status -- which synchronises `stream` and returns
 * SRGPT_ERR_UNSUPPORTED for the bit (SRGPT_ERR_STATE when more than 256 entries tied at the top-k threshold) -- reports the MOST RECENT
 * srgpt_sample call on that workspace only: check after each draw whose settings may be out of range.  Inside the decode step the
 * word is the state's own and is never cleared once raised (sticky); srgpt_llm_decode_sync_state reports it. */
int srgpt_sample_status(const void* ws, int B, srgpt_stream_t stream);
/* The full sampler (additions under ABI 9).  Two launches, capturable: (1) one 1024-thread block per sequence writes the
 * order-preserving integer keys of logits / T (a true division) to the workspace and finds the row's kept set as ONE threshold pair
 * -- the kept set is a suffix of the order (score asc, index asc): top-k by a radix select over the keys (ties at the k-th score
 * kept), top-p by the same digit walk over 64-bit fixed-point softmax mass of the top-k survivors (exact integer sums: a fixed
 * result on every replay), the lowest indices of a tie group cut by top-p removed first (CPU torch.sort's order; top_p = 0 keeps the
 * highest index among the tied maxima); (2) a masked Gumbel-max over 128 vocabulary slices (Philox addressed by (seed, counter,
 * sequence, vocabulary index)), the slices' maxima merged like the greedy argmax.  Every setting is served: no error bit.
 * ws = srgpt_sample_full_ws_bytes(B, V) = B * (4 V + 16 + 128 * 8) bytes.  kept_mask (optional, may be NULL): uint32
 * [B][ceil(V / 32)], bit i % 32 of word i / 32 set <=> entry i is kept (the parity hook).  tok_out[b] = the drawn id; advances
 * sp->counter.  V > 262144: SRGPT_ERR_UNSUPPORTED. */
int64_t srgpt_sample_full_ws_bytes(int B, int V);
int srgpt_sample_full(const float* logits, srgpt_sampling* sp, int64_t* tok_out, uint32_t* kept_mask, void* ws, int B, int V,
                      srgpt_stream_t stream);

/* Rows are steps (additions under ABI 9).  The two samplers over logits [T, V] whose rows are T SUCCESSIVE STEPS OF ONE SEQUENCE -- what
 * the sampled lookup step (srgpt_llm_lookup_step_ex) draws behind its T rows.  Row t reads the Philox stream at (counter + t,
 * sequence 0), the 64-bit sum carried into the high word; slices, selects, tie rules and the kept set are the samplers' above (the
 * kernels are the same templates, the addressing a compile-time mode).  Contract: tok_out[t] (and the kept set of row t: kept_out
 * int[T][257], kept_mask [T][ceil(V / 32)]) equals what T successive B = 1 calls of srgpt_sample / srgpt_sample_full on row t alone
 * return.  Both advance sp->counter by T.  Workspaces: srgpt_sample_ws_bytes(T), srgpt_sample_full_ws_bytes(T, V).  The error word
 * and srgpt_sample_status(ws, T, stream) behave as for srgpt_sample. */
int srgpt_sample_rows(const float* logits, srgpt_sampling* sp, int64_t* tok_out, void* ws, int T, int V, srgpt_stream_t stream);
int srgpt_sample_full_rows(const float* logits, srgpt_sampling* sp, int64_t* tok_out, uint32_t* kept_mask, void* ws, int T, int V,
                           srgpt_stream_t stream);

/* Rows are sequences x steps (additions under ABI 9).  The two samplers over logits [B * T, V] whose rows are B SEQUENCES x T SUCCESSIVE
 * STEPS, row r = b * T + t -- what the batched sampled lookup step (srgpt_llm_lookup_step_batch_ex) draws behind its rows.  The
 * sequences have emitted different numbers of ids, steps[b] (DEVICE int [B]; a negative entry counts as 0), and share ONE counter:
 * with m = min over b of max(steps[b], 0), the column of the ids every sequence has filled, sp->counter names the draw of column m,
 * and row (b, t) reads the Philox stream at (counter + (max(steps[b], 0) - m) + t, sequence b), the 64-bit sum carried into the high
 * word.  Every block computes m from steps[0 .. B) itself.  With B = 1 that is the rows-are-steps address above, with T = 1 and equal
 * steps the address of srgpt_sample / srgpt_sample_full; slices, selects, tie rules and the kept set are the samplers' (the same
 * kernel templates, the addressing a compile-time mode).
 *   Contract: tok_out[b * T + t] (and the kept set of that row: kept_out int[B * T][257], kept_mask [B * T][ceil(V / 32)]) equals
 *   what srgpt_sample / srgpt_sample_full return in row b of a B-ROW call at counter + (max(steps[b], 0) - m) + t whose row b holds
 *   these logits.
 *   Both take sp as const and leave sp->counter UNCHANGED: how far the sequences advance is the accept's decision
 *   (srgpt_llm_lookup_step_batch_ex adds the columns that filled up), not the sampler's.
 * Workspaces: srgpt_sample_ws_bytes(B * T), srgpt_sample_full_ws_bytes(B * T, V).  The error word and srgpt_sample_status(ws, B * T,
 * stream) behave as for srgpt_sample.  NULL pointers (kept_mask may be NULL), B < 1, T < 1, V < 1: SRGPT_ERR_ARG; V > 262144:
 * SRGPT_ERR_UNSUPPORTED; both before any launch. */
int srgpt_sample_seq_rows(const float* logits, const srgpt_sampling* sp, const int* steps, int64_t* tok_out, void* ws, int B, int T, int V,
                          srgpt_stream_t stream);
int srgpt_sample_full_seq_rows(const float* logits, const srgpt_sampling* sp, const int* steps, int64_t* tok_out, uint32_t* kept_mask,
                               void* ws, int B, int T, int V, srgpt_stream_t stream);

/* Logits processors (additions under ABI 9): the part of HF's `LogitsProcessorList` that `generate(repetition_penalty=...,
 * no_repeat_ngram_size=..., min_length=... / min_new_tokens=...)` builds, transformers 4.37.2 generation/logits_process.py, on the
 * device.  The parameter block lives in DEVICE memory like srgpt_sampling: one captured graph serves every setting.
 * srgpt_logits_process: scores fp32 [B, V], processed IN PLACE; ids int64 [B, ld], the first n entries of a row are that row's
 *   history (n_dev != NULL: *n_dev, a device int, replaces n -- clamped to [0, ld]).  Per row, with s = the row's scores:
 *   RepetitionPenaltyLogitsProcessor (repetition_penalty p != 1): for every DISTINCT id t of the history
 *     s[t] = s[t] < 0 ? s[t] * p : s[t] / p -- once, however often t occurs, from the ORIGINAL s[t]; a true fp32 division (the
 *     CPU's bits).
 *   NoRepeatNGramLogitsProcessor (no_repeat_ngram g > 0): when n + 1 >= g, every id t that would complete a g-gram already in the
 *     history -- some i has ids[i .. i + g - 2] equal to the last g - 1 ids and ids[i + g - 1] = t -- gets -inf (g = 1 bans every id
 *     of the history).
 *   MinLengthLogitsProcessor / MinNewTokensLengthLogitsProcessor: while n < min_new_tokens every eos[j], j < n_eos, gets -inf.  (A
 *     generate() fed `inputs_embeds` starts from empty input_ids, so both classes count generated tokens: the host passes
 *     max(min_length, min_new_tokens).)
 *   A ban (-inf) wins over a penalty on the same entry; history ids and EOS ids outside [0, V) are skipped; the result does not
 *   depend on scheduling (one block per row: every history entry reads its original score, barrier, the penalised values are
 *   written -- duplicates write identical bits --, barrier, the -inf writes).  One launch.  ld <= 12288, else SRGPT_ERR_UNSUPPORTED.
 *   NULL scores / lp / ids, B, V or ld <= 0, n outside [0, ld]: SRGPT_ERR_ARG, before any launch. */
typedef struct {
  float repetition_penalty;   /* > 0; 1.0: off */
  int   no_repeat_ngram;      /* 0: off */
  int   min_new_tokens;       /* 0: off; max(min_length, min_new_tokens) as resolved by the host */
  int   n_eos;                /* 0 .. 8 ids in eos[] */
  int64_t eos[8];
} srgpt_logits_proc;
int srgpt_logits_process(float* scores, const srgpt_logits_proc* lp, const int64_t* ids, int ld, int n, const int* n_dev, int B, int V,
                         srgpt_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Composite: vision tower (VisionTower.forward, multimodal_encoder/vision_encoder.py:115-132 over HF
 * SiglipVisionModel; returns hidden_states[select_layer], i.e. runs `n_layers_run` encoder layers).
 * All weights device pointers in `dtype`; per-layer arrays are HOST arrays of device pointers.
 * --------------------------------------------------------------------------------------------- */
typedef struct {
  int dtype, hidden, inter, heads, n_layers_run, image_size, patch, kp; /* kp: padded 3*p*p */
  int inter_pad;        /* row length of w2 and of the MLP activation buffer: inter rounded up to a multiple of 64, zero filled
                           (4304 -> 4352 for SigLIP-so400m) so that fc2's K dimension tiles exactly */
  int act;              /* MLP activation: SRGPT_ACT_GELU_TANH (SigLIP) or SRGPT_ACT_QUICK_GELU (CLIP) */
  float eps;
  const void* patch_w;  /* [hidden, kp] (conv weight flattened (c,ky,kx), zero padded) */
  const void* patch_b;  /* [hidden] or NULL (CLIP's patch conv has no bias) */
  const void* pos_emb;  /* [tokens, hidden], tokens = grid*grid (+1 with a class token) */
  const void* cls_emb;  /* [hidden] class embedding prepended to every image (CLIP) or NULL (SigLIP) */
  const void* pre_ln_w; /* CLIP pre_layrnorm (applied to the embeddings) or NULL */
  const void* pre_ln_b;
  const void* const* ln1_w; const void* const* ln1_b;
  const void* const* wqkv;  const void* const* bqkv;   /* [3*hidden, hidden] rows q;k;v */
  const void* const* wo;    const void* const* bo;
  const void* const* ln2_w; const void* const* ln2_b;
  const void* const* w1;    const void* const* b1;     /* [inter, hidden] */
  const void* const* w2;    const void* const* b2;     /* [hidden, inter_pad], columns >= inter are zero */
} srgpt_vit_weights;

/* workspace bytes for n_img images */
int64_t srgpt_vit_ws_bytes(const srgpt_vit_weights* w, int n_img);
/* rows [n_img*gg, C] patch embeddings -> x [n_img, 1+gg, C]: row 0 = cls + pos[0], row 1+p = patch p + pos[1+p]
 * (HF CLIPVisionEmbeddings.forward: cat(class_embeds, patch_embeds) + position_embedding) */
int srgpt_vit_assemble_cls(const void* patches, const void* cls_emb, const void* pos_emb, void* x, int n_img, int gg,
                           int C, int dtype, srgpt_stream_t stream);
/* images [n_img,3,S,S] -> out [n_img, tokens, hidden] */
int srgpt_vit_forward(const srgpt_vit_weights* w, const void* images, void* out, void* ws, int n_img,
                      srgpt_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Request preprocessing on the device (host originals: llava/mm_utils.py:421-474 process_image,
 * :477-532 process_regions, which use PIL, cv2 and the HF image processor).
 * srgpt_image_resize_normalize: uint8 image [H, W, C] (HWC) -> Pillow-exact bicubic resize (two uint8 passes, 22-bit
 *   fixed-point coefficients supplied by the host: per output column/row (first tap, tap count) in *bounds and
 *   *coef [out][k]) -> value * rescale -> (v - mean[c]) / std[c] if do_normalize -> out [C, Hout, Wout] in dtype.
 *   tmp_u8 = H * Wout * C bytes of scratch.  A dimension that is not resized gets the identity table (1 tap, 1<<22).
 * srgpt_mask_resize_nearest: uint8 masks [K, H, W] -> out [K, Hout, Wout] in dtype, out[m,y,x] = src[m, ys[y], xs[x]]
 *   (cv2.INTER_NEAREST index tables from the host: OpenCV resizeNN's published arithmetic, min(floor(dst * (1 / (out / in))), in - 1)
 *   in double -- pinned by tests/golden/cv2_nearest_kat.json; cv2 itself is not installed in the build image).
 * --------------------------------------------------------------------------------------------- */
int srgpt_image_resize_normalize(const void* src_u8, int H, int W, int C, const int* hbounds, const int* hcoef, int hk,
                                 const int* vbounds, const int* vcoef, int vk, int Hout, int Wout, void* tmp_u8,
                                 void* out, const float* mean, const float* stdv, float rescale, int do_normalize,
                                 int dtype, srgpt_stream_t stream);
int srgpt_mask_resize_nearest(const void* src_u8, int K, int H, int W, const int* ys, const int* xs, int Hout, int Wout,
                              void* out, int dtype, srgpt_stream_t stream);
/* ABI 6: process_regions with image_aspect_ratio == "pad" (mm_utils.py:505-531): each uint8 mask [H, W] is centred on a zero square
 * of side max(H, W) (pad_to_square: offsets (side - H) / 2, (side - W) / 2) and the HF processor resizes that one-channel square
 * to Hout x Wout with Pillow's bicubic filter, rescale_factor 1.0, no normalisation.  masks [K, H, W] -> out [K, Hout, Wout] in
 * dtype (values 0 .. 255 as the uint8 result holds them); *bounds / *coef are Pillow's tables for side -> Wout (h) and side -> Hout
 * (v) as for srgpt_image_resize_normalize; tmp_u8 = K * side * Wout bytes.  The padded square is never materialised. */
int srgpt_mask_pad_resize(const void* src_u8, int K, int H, int W, const int* hbounds, const int* hcoef, int hk,
                          const int* vbounds, const int* vcoef, int vk, int Hout, int Wout, void* tmp_u8, void* out,
                          int dtype, srgpt_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Composite: Llama decoder (LlamaForCausalLM.forward, modeling_llama.py:972-1110 inference branch,
 * LlamaModel.forward :824-936, LlamaDecoderLayer :611-684) with a static KV cache.
 * --------------------------------------------------------------------------------------------- */
typedef struct {
  int dtype, hidden, inter, layers, heads, kv_heads, head_dim, vocab;
  float rms_eps;
  /* ABI 9: MXFP4 weights only (wqkv4 below).  0: srgpt_llm_prefill, _ragged and _append run the plain srgpt_gemm_w4 entries.  1: they
   * run the `_direct` entries -- q/k/v, gate/up and down_proj of a 225 .. 272-row prefill multiply the codes in the whole-M kernel, no
   * bf16 expansion; every byte written is the same.  Any other value, or 1 without wqkv4: SRGPT_ERR_ARG from every LLM entry point.
   * The field sits in the four bytes that padded rms_eps in front of the pointer below: no offset and no size of the struct changed,
   * and a zero-initialised struct is the behaviour before the field. */
  int mxfp4_direct;
  const void* rope_cos;    /* [max_pos, head_dim/2] (see srgpt_rope_kv_append) */
  const void* rope_sin;
  const void* embed;       /* [vocab, hidden] */
  const void* final_norm;  /* [hidden] */
  const void* lm_head;     /* [vocab, hidden] */
  const void* const* attn_norm; /* per layer [hidden] */
  const void* const* wqkv;      /* per layer [(heads+2*kv_heads)*head_dim, hidden]  rows q;k;v */
  const void* const* wo;        /* per layer [hidden, heads*head_dim] */
  const void* const* mlp_norm;  /* per layer [hidden] */
  const void* const* wgu;       /* per layer [2*inter, hidden]  rows gate;up */
  const void* const* wdown;     /* per layer [hidden, inter] */
  /* Optional fp8 (OCP e4m3fn) copies + per-row fp32 scales of the five streamed matrices.  When wqkv8 != NULL the DECODE
   * step streams these through srgpt_gemv_w8 (half the bytes per token) and prefill multiplies them with srgpt_gemm_w8; the
   * dtype matrices above (wqkv / wo / wgu / wdown / lm_head) are then never read and may be NULL (per-layer arrays of NULLs):
   * the fp8 bytes are the only copy of those weights in HBM. */
  const void* lm_head8;
  const float* lm_head_scale;
  const void* const* wqkv8;
  const float* const* wqkv_scale;
  const void* const* wo8;
  const float* const* wo_scale;
  const void* const* wgu8;
  const float* const* wgu_scale;
  const void* const* wdown8;
  const float* const* wdown_scale;
  /* fp8 or MXFP4 weights.  0: bf16 activations everywhere (W8A16 / W4A16: exact weights x bf16 activations -- the default, what the
   * parity tests pin).  1: prefill, ragged prefill and append prefill quantise each GEMM's input per token (srgpt_quant_rows_e4m3) and
   * multiply on the fp8 matrix pipe -- srgpt_gemm_w8a8 with fp8 weights, srgpt_gemm_w4a8 with MXFP4 weights (wqkv4 below: W4A8, the
   * codes times the block scales in the instruction, no bf16 expansion at any row count; mxfp4_direct is then not consulted and the
   * workspace holds no expansion scratch).  Decode steps and the all-position lm_head keep bf16 activations.  Needs hidden, inter and
   * heads * head_dim % 128 == 0 (>= 256), else the prefill entries return SRGPT_ERR_UNSUPPORTED. */
  int fp8_act;
  /* ABI 9: rows per weight pass of the decode step's MFMA products.  0 or 16: passes of 16 rows.  32: the wide pass above (the step
   * calls srgpt_gemv_rowss_wide / srgpt_gemv_w4p_wide) -- a step of 17 - 32 rows reads every weight byte once.  Any other value:
   * SRGPT_ERR_ARG from every LLM entry point.  The field sits in the four bytes that padded fp8_act in front of the pointer below: no
   * offset and no size of the struct changed, and a zero-initialised struct is the behaviour before the field. */
  int decode_pass_rows;
  /* ABI 9: optional PACKED copies (srgpt_pack_decode_weights) of the fp8 layer matrices for the batched decode step (2+ rows per GPU);
   * NULL (array or entry): that product streams the row-major copy.  pk_rows_*: rows per granule of the matrix' packed copies. */
  const void* const* wqkv8p;
  const void* const* wo8p;
  const void* const* wgu8p;
  const void* const* wdown8p;
  int pk_rows_qkv, pk_rows_o, pk_rows_gu, pk_rows_down;
  /* ABI 9: optional MXFP4 copies (codes + E8M0 block scales, see srgpt_gemv_w4) of the four per-layer matrices; all NULL: the formats
   * above.  When wqkv4 != NULL they are the weights of those four (the dtype and fp8 arrays above are not read for them and may hold
   * NULLs): the decode step, the lookup steps included, streams them through srgpt_gemv_w4 (a batch of more than 4 rows in passes of
   * 4); prefill and append prefill run the srgpt_gemm_w4 family -- bit-identical to a bf16 engine on the dequantised weights: the
   * direct-to-LDS kernels (every product of an append, o_proj of the bs = 1 prefill) multiply the codes themselves, the whole-M and
   * 256 x 256 routes still expand each matrix with srgpt_dequant_mxfp4 into a bf16 scratch in the workspace just before its product,
   * at the price of one more pass over bf16-sized bytes per such matrix.  With fp8_act = 1 (above) the prefill entries are W4A8
   * instead: per-token e4m3 activations x the codes on the block-scaled MFMA (srgpt_gemm_w4a8), nothing expanded; the decode steps are
   * the same W4A16 ones.  lm_head stays fp8: lm_head8 + lm_head_scale are required, multiplied as under the fp8
   * format.  Needs dtype SRGPT_BF16, hidden, inter and heads * head_dim multiples of 32, and wqkv8 == NULL. */
  const void* const* wqkv4;
  const void* const* wqkv4_scale;
  const void* const* wo4;
  const void* const* wo4_scale;
  const void* const* wgu4;
  const void* const* wgu4_scale;
  const void* const* wdown4;
  const void* const* wdown4_scale;
} srgpt_llm_weights;

typedef struct {
  int batch, max_pos;
  void* kcache;   /* [layers, batch, kv_heads, max_pos, head_dim] */
  void* vcache;
  int* pos;       /* device int[batch]: tokens already in the cache */
  int64_t* tok;   /* device int64[batch]: next input token id (decode) */
  int64_t* out_ids; /* device int64[batch, max_new]: generated ids, column = *step */
  int* step;      /* device int[1]: decode step counter */
  int max_new;
  int ws_tokens;  /* max prompt tokens per sequence the workspace was sized for */
  void* ws;       /* workspace, srgpt_llm_ws_bytes(w, batch, ws_tokens).  It holds the decode attention's arrival tickets, which
                   * must be zero before a decode step: every srgpt_llm_prefill* zeroes them (so a hipMalloc'ed, never-zeroed
                   * workspace is fine as long as a prefill precedes the first step, which it must anyway) */
  float* logits;  /* [batch, vocab] fp32 (last position) */
  srgpt_sampling* sampling; /* ABI 6: DEVICE pointer or NULL.  NULL: greedy (argmax).  Set: srgpt_llm_sample_first / srgpt_llm_decode_step
                             * and the graphs captured from this state DRAW the next token (see srgpt_sampling) */
} srgpt_llm_state;

/* (MXFP4 weights: plus one bf16 scratch for the largest of the four layer matrices; every other format: unchanged) */
int64_t srgpt_llm_ws_bytes(const srgpt_llm_weights* w, int batch, int max_tokens);
/* Prefill: inputs_embeds [B, T, hidden] (already spliced), all rows valid (equal-length prompts).
 * Fills the cache, sets pos[b] = T, writes last-position logits to st->logits; if all_logits != NULL
 * also writes fp32 logits for every position [B, T, vocab]; if hidden_out != NULL writes the
 * (layers+1) pre-norm hidden states [layers+1, B, T, hidden] (parity hook). */
int srgpt_llm_prefill(const srgpt_llm_weights* w, srgpt_llm_state* st, const void* inputs_embeds, int T,
                      float* all_logits, void* hidden_out, srgpt_stream_t stream);
/* Ragged batch (prompts of different lengths in one call -- the reference right-pads and hands flash-attn the unpadded
 * rows, llava_arch.py:549-611 + modeling_llama.py:540-608): inputs_embeds [batch, T, hidden] RIGHT-padded, lens[b] =
 * valid rows of sequence b (device int32).  Causal attention never looks right, so valid rows are exact whatever the
 * padding holds; logits come from row lens[b]-1 and decoding continues at position lens[b] per sequence. */
int srgpt_llm_prefill_ragged(const srgpt_llm_weights* w, srgpt_llm_state* st, const void* inputs_embeds, int T,
                             const int* lens, float* all_logits, void* hidden_out, srgpt_stream_t stream);
/* Append prefill (additions under ABI 9): continue every sequence of a LIVE state with a multi-token segment -- HF's cached forward
 * over input_ids [B, T > 1] (modeling_llama.py:398-456; the caller's side: llava_arch.py:355-385), the next turn of a conversation
 * or the next question over a shared prefix without re-running the rows already in the cache.
 *   inputs_embeds [batch, T, hidden] RIGHT-padded; lens (device int[batch], NULL = T each) = rows to append per sequence, 1 .. T.
 *   Row b continues at st->pos[b].  h_pos_max is a HOST int: the caller's upper bound on every st->pos[b] on entry (the call is
 *   checked and sized without a synchronisation): T outside 1 .. ws_tokens, h_pos_max < 0 or h_pos_max + T > max_pos is
 *   SRGPT_ERR_ARG before any launch.  The first launch validates every row on the device (0 <= pos[b] <= h_pos_max,
 *   1 <= lens[b] <= T); a violating row raises the state's sticky error word (srgpt_llm_decode_sync_state: SRGPT_ERR_STATE) and is
 *   appended at a clamped position: whatever st->pos holds, no byte outside the cache is written.
 *   The launches are srgpt_llm_prefill's (every weight format) with the per-row positions in the RoPE / append and attention calls;
 *   on a state whose rows are all at position 0 (lens NULL, h_pos_max 0) every byte written equals srgpt_llm_prefill's.
 *   Afterwards pos[b] += lens[b], st->logits holds row lens[b] - 1 of every sequence, all_logits [batch, T, vocab] and hidden_out
 *   [layers + 1, batch, T, hidden] (optional) the NEW rows.  A captured decode step re-embeds st->tok after this call.  The error
 *   word is NOT cleared and the decode tickets are not touched (only a prefill re-arms them).  Cache rows pos[b] + lens[b] .. pos[b] +
 *   T - 1 of a padded sequence receive the padding's k / v: they lie beyond the live length and the next append overwrites them. */
int srgpt_llm_prefill_append(const srgpt_llm_weights* w, srgpt_llm_state* st, const void* inputs_embeds, int T, const int* lens,
                             int h_pos_max, float* all_logits, void* hidden_out, srgpt_stream_t stream);
/* One greedy decode step, entirely device-side: embeds st->tok, runs the layers against the cache,
 * argmax -> st->tok, st->out_ids[:, *step], ++pos, ++*step.  No host sync. */
int srgpt_llm_decode_step(const srgpt_llm_weights* w, srgpt_llm_state* st, srgpt_stream_t stream);
/* Health check of the decode steps since the last prefill (synchronises `stream` once): 0 when every arrival ticket of the decode
 * attention in st->ws is re-armed (zero), no captured step met a caller-written token id outside the embedding table and no
 * srgpt_llm_prefill_append met a row outside its host bounds; SRGPT_ERR_STATE otherwise (srgpt_last_error says which). */
int srgpt_llm_decode_sync_state(const srgpt_llm_weights* w, const srgpt_llm_state* st, srgpt_stream_t stream);
/* first token after prefill: argmax(st->logits) -> tok / out_ids[:,0] / step=1 */
int srgpt_llm_sample_first(const srgpt_llm_weights* w, srgpt_llm_state* st, srgpt_stream_t stream);

/* hipGraph capture of one decode step (replayed per token; removes per-launch host cost).  A replay continues from st->tok: normally
 * the token the step before it (srgpt_llm_decode_step, srgpt_llm_sample_first or the previous replay) picked, whose embedding row
 * that step already left in the residual-stream workspace; the captured step's first node compares st->tok with the token that row
 * belongs to and re-embeds when the caller wrote a token of its own into st->tok between replays; an id outside the table cannot be
 * embedded -- the step then runs on the previous row and raises a sticky error that srgpt_llm_decode_sync_state reports. */
typedef struct srgpt_graph srgpt_graph;
int srgpt_llm_decode_graph_create(const srgpt_llm_weights* w, srgpt_llm_state* st, srgpt_stream_t stream,
                                  srgpt_graph** out);
/* Sampler kinds of the _ex forms (additions under ABI 9): which device sampler draws when st->sampling is set (greedy otherwise,
 * whatever the kind).  The forms without _ex are the SRGPT_SAMPLER_TOPK64 case.  An unknown kind is SRGPT_ERR_ARG; the full sampler
 * over a vocabulary above 262144 is SRGPT_ERR_UNSUPPORTED -- both before any launch.  A graph captured with one kind replays that
 * kind; the parameter block still says which setting. */
enum { SRGPT_SAMPLER_TOPK64 = 0, SRGPT_SAMPLER_FULL = 1 };
int srgpt_llm_sample_first_ex(const srgpt_llm_weights* w, srgpt_llm_state* st, int sampler, srgpt_stream_t stream);
int srgpt_llm_decode_step_ex(const srgpt_llm_weights* w, srgpt_llm_state* st, int sampler, srgpt_stream_t stream);
int srgpt_llm_decode_graph_create_ex(const srgpt_llm_weights* w, srgpt_llm_state* st, int sampler, srgpt_stream_t stream,
                                     srgpt_graph** out);
/* The _ex forms with logits processors (additions under ABI 9).  lp: DEVICE pointer to a srgpt_logits_proc block, or NULL = exactly
 * the _ex form (same launches).  With lp set, srgpt_logits_process runs on st->logits between lm_head and the pick -- in front of the
 * greedy argmax and of both samplers -- with ids = st->out_ids, ld = st->max_new and the count read from st->step on the device: the
 * first token (srgpt_llm_sample_first_proc) sees 0 ids whatever *step held before, step t sees the t ids generated so far.
 * st->logits holds the PROCESSED scores after such a step.  st->max_new > 12288 with lp set: SRGPT_ERR_UNSUPPORTED before any
 * launch.  A graph captured with lp replays with that block's address; the block's contents may change between replays. */
int srgpt_llm_sample_first_proc(const srgpt_llm_weights* w, srgpt_llm_state* st, int sampler, const srgpt_logits_proc* lp,
                                srgpt_stream_t stream);
int srgpt_llm_decode_step_proc(const srgpt_llm_weights* w, srgpt_llm_state* st, int sampler, const srgpt_logits_proc* lp,
                               srgpt_stream_t stream);
int srgpt_llm_decode_graph_create_proc(const srgpt_llm_weights* w, srgpt_llm_state* st, int sampler, const srgpt_logits_proc* lp,
                                       srgpt_stream_t stream, srgpt_graph** out);
int srgpt_graph_launch(srgpt_graph* g, int times, srgpt_stream_t stream);
int srgpt_graph_destroy(srgpt_graph* g);

/* ---------------------------------------------------------------------------------------------
 * Prompt-lookup decoding (additions under ABI 9): HF generate(prompt_lookup_num_tokens = K) -- transformers 4.37
 * generation/candidate_generator.py PromptLookupCandidateGenerator + GenerationMixin.assisted_decoding, greedy and (the _ex forms at
 * the end of this section) sampled.  A decode step is
 * weight-bound: its cost barely depends on the rows riding through it.  The lookup step carries T = K + 1 rows of ONE sequence -- the
 * next token and K ids drafted from the sequence itself -- and emits 1 .. T tokens, the same ids the plain greedy loop emits.
 *
 * srgpt_lookup_draft (one block): the history is prompt_ids[n_prompt] (int64, may be NULL when n_prompt = 0) followed by the first
 *   *step ids of out_ids (step: device int, clamped to 0 .. max_new).  An id outside [0, vocab) is a sentinel (-200): it never matches
 *   and is never drafted.  For n = min(max_ngram, len - 1) down to 1: take the last n ids; find the EARLIEST earlier occurrence that
 *   has a (non-sentinel) id after it; the up to K non-sentinel ids that follow are draft[0 .. *n_draft) (the rest of draft[K] is -1;
 *   *n_draft = 0: no match).  The position is a minimum over the matches: the result does not depend on scheduling.
 *   K 1 .. 15, max_ngram 1 .. 8, else SRGPT_ERR_ARG.
 * srgpt_lookup_accept (one block): picks int64 [T] = the model's greedy pick behind each of the T rows (srgpt_argmax).  n_acc = the
 *   longest prefix with draft[i] == picks[i], i < *n_draft (and pos[0] + i + 1 < max_pos).  The step emits picks[0 .. n_acc]: they go
 *   to out_ids[*step ..], cut at max_new; *step and pos[0] advance by the number emitted, tok[0] = the last one emitted, tok_emb[0]
 *   (optional) = -1, stats[3] (optional, device ints) += {1, *n_draft, n_acc}.  *step >= max_new on entry: nothing changes (a
 *   run-ahead loop may launch once too often).  T 2 .. 16.
 * --------------------------------------------------------------------------------------------- */
int srgpt_lookup_draft(const int64_t* prompt_ids, int n_prompt, const int64_t* out_ids, const int* step, int max_new, int K,
                       int max_ngram, int64_t vocab, int64_t* draft, int* n_draft, srgpt_stream_t stream);
int srgpt_lookup_accept(const int64_t* picks, const int64_t* draft, const int* n_draft, int T, int64_t* tok, int64_t* out_ids,
                        int* pos, int* step, int max_new, int max_pos, int64_t* tok_emb, int* stats, srgpt_stream_t stream);

/* The lookup step's parameter block (HOST struct of device pointers; a captured graph keeps the addresses). */
typedef struct {
  int T;                     /* rows per step = K + 1, 2 .. 16; on the bf16 matrix-pipe attention T * heads / kv_heads <= 16 */
  int max_ngram;             /* HF max_matching_ngram_size (default 2), 1 .. 8 */
  const int64_t* prompt_ids; /* the request's input_ids row as the caller gave it (sentinels included), or NULL */
  int n_prompt;
  void* ws;                  /* srgpt_llm_lookup_ws_bytes(w, T) bytes, ZEROED once when allocated (it holds arrival tickets) */
  float* logits;             /* [T, vocab] fp32: the logits behind each of the T rows */
  int* stats;                /* device int[3]: steps, drafted, accepted -- incremented by every step */
} srgpt_lookup;

/* workspace bytes of a T-row lookup step: T rows of the decode step's buffers, two row-statistics tables, the workspace of
 * srgpt_decode_attention_multi, the rows' pick partials and the draft scratch.  (srgpt_llm_ws_bytes does not change.) */
int64_t srgpt_llm_lookup_ws_bytes(const srgpt_llm_weights* w, int T);
/* One lookup step of a batch-1 GREEDY state, entirely device-side: srgpt_lookup_draft over (lk->prompt_ids, st->out_ids) -> the T
 * rows' embeddings (st->tok, the drafts, then the last id repeated -- rows that can never be accepted) -> the layers of
 * srgpt_llm_decode_step with T rows through the same products (bf16, W8A16 and the packed fp8 copies) and
 * srgpt_decode_attention_multi -> lm_head into lk->logits -> the rows' argmax -> srgpt_lookup_accept on the state.  It equals that
 * composition of the per-op entries bit for bit, and row 0 -- hence every emitted id -- does not depend on the drafts.
 * st->sampling set (the sampled step is the _ex form below), T beyond the attention's columns or 16: SRGPT_ERR_UNSUPPORTED; batch != 1, T < 2, NULL pointers: SRGPT_ERR_ARG;
 * all before any launch.  Cache rows behind the accepted ones hold rejected drafts: they lie beyond st->pos and the next step
 * overwrites them.  A plain captured step may follow (tok_emb = -1 makes it re-embed st->tok).
 * srgpt_llm_lookup_graph_create captures one step; replay with srgpt_graph_launch.
 * srgpt_llm_lookup_sync_state: srgpt_llm_decode_sync_state for such a state -- the lookup workspace's own arrival tickets are checked
 * first (SRGPT_ERR_STATE), then the plain check runs unchanged. */
int srgpt_llm_lookup_step(const srgpt_llm_weights* w, srgpt_llm_state* st, const srgpt_lookup* lk, srgpt_stream_t stream);
int srgpt_llm_lookup_graph_create(const srgpt_llm_weights* w, srgpt_llm_state* st, const srgpt_lookup* lk, srgpt_stream_t stream,
                                  srgpt_graph** out);
int srgpt_llm_lookup_sync_state(const srgpt_llm_weights* w, const srgpt_llm_state* st, const srgpt_lookup* lk, srgpt_stream_t stream);
/* The lookup step under SAMPLING (additions under ABI 9).  Prompt lookup has no draft distribution, so this is HF's assisted decoding
 * without candidate logits: one token is drawn from the warped distribution behind each of the T rows, the drafts are kept up to the
 * first draw that differs, and that draw is emitted.  It is exact: row t's draw is used only when rows 0 .. t - 1 agreed, so it is a
 * draw from the model's distribution behind the emitted prefix.
 *   With st->sampling == NULL the _ex forms ARE the greedy step above (same launches; sample_ws may be NULL).  With st->sampling set
 *   the step is the same through lm_head into lk->logits; then the sampler `sampler` (SRGPT_SAMPLER_*) runs in its rows-are-steps mode
 *   over the T rows -- row t draws at Philox counter sp->counter + t, as srgpt_sample_rows / srgpt_sample_full_rows; its error bits go
 *   to the state's sticky error word (srgpt_llm_decode_sync_state) -- and the accept takes the draws for picks and does
 *   sp->counter += the ids emitted (0 when *st->step >= max_new on entry).  Generated id i is therefore drawn at counter c0 + i, as in
 *   the plain sampled loop; a discarded row's random numbers influenced nothing that was kept.
 *   sample_ws: srgpt_llm_lookup_sample_ws_bytes(w, T, sampler) bytes = srgpt_sample_ws_bytes(T) / srgpt_sample_full_ws_bytes(T, vocab)
 *   (-1: T outside 2 .. 16, unknown kind, NULL weights).  Unknown sampler kind, or st->sampling set with sample_ws NULL: SRGPT_ERR_ARG;
 *   every refusal of srgpt_llm_lookup_step but the greedy-only one applies; all before any launch.  A graph captured with st->sampling
 *   set replays the sampled step of that kind.  srgpt_llm_lookup_sync_state serves both steps. */
int64_t srgpt_llm_lookup_sample_ws_bytes(const srgpt_llm_weights* w, int T, int sampler);
int srgpt_llm_lookup_step_ex(const srgpt_llm_weights* w, srgpt_llm_state* st, const srgpt_lookup* lk, int sampler, void* sample_ws,
                             srgpt_stream_t stream);
int srgpt_llm_lookup_graph_create_ex(const srgpt_llm_weights* w, srgpt_llm_state* st, const srgpt_lookup* lk, int sampler,
                                     void* sample_ws, srgpt_stream_t stream, srgpt_graph** out);

/* The lookup step for a BATCH (additions under ABI 9): B = st->batch sequences of T = K + 1 rows each ride through one pass over the
 * weights.  Every sequence is drafted from its OWN history, verified in the shared step and advanced by its OWN number of accepted
 * drafts; greedy here, sampled through the _ex forms at the end of this header.  Row r = b * T + t of every step buffer is token t of sequence b, the [B, T, ...] layout of
 * srgpt_decode_attention_multi.  B * T <= 16: the rows one pass of the decode products' MFMA kernel carries.  The entry points above
 * are unchanged and keep refusing a state of more than one sequence.
 *
 * srgpt_lookup_draft_batch (B blocks): srgpt_lookup_draft per sequence.  The history of sequence b is prompt_ids[b, 0 .. n_prompt[b])
 *   (int64 rows of stride ld_prompt, every row's ids packed to the front; n_prompt: DEVICE int [B], clamped to 0 .. ld_prompt;
 *   prompt_ids may be NULL when ld_prompt = 0) followed by the first steps[b] ids of out_ids[b, :] (out_ids int64 [B, max_new], steps:
 *   device int [B], each clamped to 0 .. max_new).  draft int64 [B, K], n_draft int [B].  B 1 .. 16, K and max_ngram as above.
 * srgpt_lookup_accept_batch (one block): picks int64 [B * T].  Sequence b takes srgpt_lookup_accept's rule on its own steps[b],
 *   pos[b], tok[b], tok_emb[b] (optional), out_ids[b, :], draft[b, :] (row stride T - 1), n_draft[b] and picks[b * T ..], the clamp
 *   pos[b] + i + 1 < max_pos included.  A sequence with steps[b] >= max_new is FROZEN: nothing of it is written or counted (it
 *   accepted more than the others and waits for them).  Then *step = min over b of steps[b], the number of columns of out_ids every
 *   sequence has filled -- the meaning *st->step has everywhere else -- and stats[3] (optional) += {1, the drafts, the accepted
 *   drafts} summed over the sequences that advanced ({0, 0, 0} when every one is frozen).  B * T <= 16, else SRGPT_ERR_UNSUPPORTED.
 * --------------------------------------------------------------------------------------------- */
int srgpt_lookup_draft_batch(const int64_t* prompt_ids, int ld_prompt, const int* n_prompt, const int64_t* out_ids, const int* steps,
                             int B, int max_new, int K, int max_ngram, int64_t vocab, int64_t* draft, int* n_draft,
                             srgpt_stream_t stream);
int srgpt_lookup_accept_batch(const int64_t* picks, const int64_t* draft, const int* n_draft, int B, int T, int64_t* tok,
                              int64_t* out_ids, int* pos, int* steps, int* step, int max_new, int max_pos, int64_t* tok_emb, int* stats,
                              srgpt_stream_t stream);

/* The batched lookup step's parameter block (HOST struct of device pointers; a captured graph keeps the addresses). */
typedef struct {
  int T;                     /* rows per sequence = K + 1 >= 2; st->batch * T <= 16, and T * heads / kv_heads <= 16 on the bf16 matrix-pipe attention */
  int max_ngram;             /* longest trailing n-gram the matcher compares, 1 .. 8 */
  const int64_t* prompt_ids; /* int64 [B, ld_prompt]: every sequence's ids (sentinels included) packed to the front of its row; NULL when ld_prompt = 0 */
  int ld_prompt;             /* row stride of prompt_ids, >= 0 */
  const int* n_prompt;       /* device int [B]: ids in every row */
  int* steps;                /* device int [B]: ids sequence b has emitted; the caller sets every entry to 1 behind srgpt_llm_sample_first */
  void* ws;                  /* srgpt_llm_lookup_batch_ws_bytes(w, B, T) bytes, ZEROED once when allocated (it holds arrival tickets) */
  float* logits;             /* [B * T, vocab] fp32: the logits behind each row */
  int* stats;                /* device int[3]: steps, drafted, accepted -- incremented by every step that advanced a sequence */
} srgpt_lookup_batch;

/* workspace bytes of a batched lookup step: B * T rows of what srgpt_llm_lookup_ws_bytes counts per row, the workspace of
 * srgpt_decode_attention_multi for (B, T), and [B, T] draft scratch.  -1: NULL weights, B < 1, T < 2 or B * T > 16. */
int64_t srgpt_llm_lookup_batch_ws_bytes(const srgpt_llm_weights* w, int B, int T);
/* One batched lookup step of a GREEDY state, entirely device-side: srgpt_lookup_draft_batch over (lk->prompt_ids, st->out_ids,
 * lk->steps) -> the B * T rows' embeddings (per sequence: st->tok[b], its drafts, then the last id repeated) -> the layers of
 * srgpt_llm_decode_step with B * T rows through the same products and srgpt_decode_attention_multi with B sequences at st->pos[b] ->
 * lm_head into lk->logits -> the rows' argmax -> srgpt_lookup_accept_batch on the state and lk->steps (*st->step = min steps[b]).
 * It equals that composition of the per-op entries bit for bit; with one sequence it leaves the bits srgpt_llm_lookup_step leaves.
 * st->sampling set, st->batch * T > 16 (the message names both), T beyond the attention's columns: SRGPT_ERR_UNSUPPORTED; T < 2, NULL
 * pointers, ld_prompt < 0: SRGPT_ERR_ARG; all before any launch.  A sequence the caller has finished keeps stepping until its
 * steps[b] reaches st->max_new, like a finished row of the plain batched loop; st->pos of sequences that ran ahead is the caller's
 * to roll back.  A plain captured step may follow.
 * srgpt_llm_lookup_graph_create_batch captures one step; replay with srgpt_graph_launch.
 * srgpt_llm_lookup_sync_state_batch: srgpt_llm_lookup_sync_state for such a state -- the (B, T) lookup workspace's arrival tickets
 * (SRGPT_ERR_STATE), then srgpt_llm_decode_sync_state (the state's tickets and its sticky error word). */
int srgpt_llm_lookup_step_batch(const srgpt_llm_weights* w, srgpt_llm_state* st, const srgpt_lookup_batch* lk, srgpt_stream_t stream);
int srgpt_llm_lookup_graph_create_batch(const srgpt_llm_weights* w, srgpt_llm_state* st, const srgpt_lookup_batch* lk,
                                        srgpt_stream_t stream, srgpt_graph** out);
int srgpt_llm_lookup_sync_state_batch(const srgpt_llm_weights* w, const srgpt_llm_state* st, const srgpt_lookup_batch* lk,
                                      srgpt_stream_t stream);

/* The batched lookup step under SAMPLING (additions under ABI 9): the _ex forms of the three entries above, in the manner of
 * srgpt_llm_lookup_step_ex.  With st->sampling == NULL they ARE the greedy batched step (same launches; sample_ws may be NULL).  With
 * st->sampling set the step is the same through lm_head into lk->logits; then the sampler `sampler` (SRGPT_SAMPLER_*) runs in its
 * sequences-x-steps mode over the B * T rows with lk->steps as its counts (srgpt_sample_seq_rows / srgpt_sample_full_seq_rows; its
 * error bits go to the state's sticky error word), and the accept takes the draws for picks: every sequence by srgpt_lookup_accept_batch's
 * rule, *st->step = min steps[b] and the stats as there, and sp->counter += m_after - m_before, m = min over b of max(steps[b], 0)
 * before and after -- 0 when every sequence is frozen.  So sp->counter keeps naming the draw of the column every sequence has filled
 * (behind srgpt_llm_sample_first_ex: counter = c0 + 1 with every steps[b] = 1), and generated id i of sequence b is drawn at
 * (c0 + i, b) as in the plain sampled batched loop, however many drafts the steps accepted; a discarded row's random numbers
 * influenced nothing that was kept.  It is exact as srgpt_llm_lookup_step_ex is: row t's draw is used only when rows 0 .. t - 1 of
 * its sequence agreed with their drafts.  With one sequence it leaves the bits srgpt_llm_lookup_step_ex leaves.
 *   sample_ws: srgpt_llm_lookup_batch_sample_ws_bytes(w, B, T, sampler) bytes = srgpt_sample_ws_bytes(B * T) /
 *   srgpt_sample_full_ws_bytes(B * T, vocab) (-1: NULL weights, B < 1, T < 2, B * T > 16, unknown kind).  Unknown sampler kind, or
 *   st->sampling set with sample_ws NULL: SRGPT_ERR_ARG; every refusal of srgpt_llm_lookup_step_batch but the greedy-only one applies;
 *   all before any launch.  srgpt_llm_lookup_step_batch itself keeps refusing a sampling state.  A graph captured with st->sampling
 *   set replays the sampled step of that kind.  srgpt_llm_lookup_sync_state_batch serves both steps. */
int64_t srgpt_llm_lookup_batch_sample_ws_bytes(const srgpt_llm_weights* w, int B, int T, int sampler);
int srgpt_llm_lookup_step_batch_ex(const srgpt_llm_weights* w, srgpt_llm_state* st, const srgpt_lookup_batch* lk, int sampler,
                                   void* sample_ws, srgpt_stream_t stream);
int srgpt_llm_lookup_graph_create_batch_ex(const srgpt_llm_weights* w, srgpt_llm_state* st, const srgpt_lookup_batch* lk, int sampler,
                                           void* sample_ws, srgpt_stream_t stream, srgpt_graph** out);

#ifdef __cplusplus
}
#endif
#endif /* SRGPT_H_ */
