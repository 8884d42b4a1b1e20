// Every function that crosses translation units inside the library and is NOT part of the C ABI (include/srgpt.h) is declared
// here, once: the file that defines it and every file that calls it include this header, so the compiler checks the definition
// against the declaration.  These are C++ functions: exports.map keeps their (mangled) names out of the dynamic symbol table,
// which holds what include/srgpt.h declares and nothing else (tests/test_capi_symbols.py).  (srgpt_set_error is in common.h,
// beside the macros that call it.)
#pragma once
#include "common.h"

struct SrgptGemmEpilogue;  // gemm_epilogue.h
struct GemmRoute;          // gemm_route.h
struct AttnPrefillRoute;   // attn_route.h

// ---- gemm256.hip / gemm288.hip: the 256 x 256 and the whole-M (up to 272 rows) bf16 MFMA tiles, dispatched by gemm.hip ----
int srgpt_gemm256_launch(const void* A, const void* W, int K, int lda, const SrgptGemmEpilogue& e, hipStream_t s);
int srgpt_gemm288_launch(const void* A, const void* W, int K, int lda, const SrgptGemmEpilogue& e, hipStream_t s);
// its W4 instance: MXFP4 codes [N, K / 2] + E8M0 bytes [N, K / 32] as the weight operand, where gemm_route.h's
// gemm_w4_direct_in_kernel / gemm_swiglu_w4_direct_in_kernel say so (SRGPT_ERR_ARG before any launch otherwise)
int srgpt_gemm288_w4_launch(const void* A, const void* W4, const void* wscale8, int K, int lda, const SrgptGemmEpilogue& e,
                            hipStream_t s);

// ---- gemm.hip: split-K around a product's launch, for every GEMM launcher (gemm.hip, gemm_f8.hip): the route's split into the
//      epilogue in front of it, the slab reduction + epilogue (when K was split) behind it; *fused (may be NULL) = the norm / RoPE
//      of the epilogue went into the reduction ----
void srgpt_splitk_apply(SrgptGemmEpilogue& e, const GemmRoute& r, void* ws);
int srgpt_splitk_finish(const SrgptGemmEpilogue& e, hipStream_t s, bool* fused);

// ---- the decode products (gemv.hip, gemv_w8.hip, gemv_w4.hip, gemv_w4p.hip, skinny.hip; gemv_p13.hip is one row, one launch) ----
// The VALU kernels share their x-staging prologue, their lane-0 epilogue and their launch tail (gemv_valu.h); every entry point
// validates its own arguments, takes its route from gemv_route.h and goes through the one pass loop below.
// One product as its entry point received it.  W: dtype weights, or (fp8) e4m3 bytes with wscale, row-major or packed (`packed` rows
// per granule), or MXFP4 codes with wscale8, or (w4) their packed array; ss_in / ss_out: the rows' statistics tables of
// srgpt_gemv_rowss, or NULL
struct DecodeProduct {
  const void *x, *W;
  const float* wscale;
  const void* norm_w;
  float eps;
  const void* residual;
  void* out;
  int batch, N, K, swiglu, out_f32, dtype, fp8;
  const float* ss_in;
  float* ss_out;
  int packed;
  int w4;  // W is a packed MXFP4 array (srgpt_pack_mxfp4) of `packed` rows per granule: srgpt_skinny_launch only (gemv_w4p.hip)
  const unsigned char* wscale8;  // W is a row-major MXFP4 code array, these its E8M0 block scales: srgpt_gemv_w4_valu only
};
// gemv.hip: the way in for validated arguments -- cuts the call into the route's weight passes and hands every pass (`batch` = its
// rows) to the launcher of the route's family.  Without a route: gemv_route's (srgpt_gemv, srgpt_gemv_w8, srgpt_gemv_rowss);
// srgpt_gemv_w4 and srgpt_gemv_w4p bring gemv_w4_route's and gemv_w4_step_route's
int srgpt_decode_product(const DecodeProduct& p, const GemvRoute& r, hipStream_t s);
int srgpt_decode_product(const DecodeProduct& p, hipStream_t s);
int srgpt_skinny_launch(const DecodeProduct& p, hipStream_t s);  // skinny.hip: MFMA, up to 16 bf16 rows; bf16, fp8 or packed MXFP4 weights
int srgpt_gemv_w8_valu(const DecodeProduct& p, hipStream_t s);   // gemv_w8.hip: VALU, one row, fp8 weights (K % 16 == 0)
int srgpt_gemv_w4_valu(const DecodeProduct& p, hipStream_t s);   // gemv_w4.hip: VALU, up to W4_MAX_ROWS rows, MXFP4 weights

// ---- pack13.hip: the binding table of the 13-bit packed copies (pack13_bind.h), for the decode-layer sequence of model.hip: the
//      binding srgpt_pack13_bind made for the raw matrix at W_raw, if it has exactly this shape ----
struct Pack13Binding;
bool srgpt_pack13_lookup(const void* W_raw, int rows, int K, Pack13Binding* out);

// ---- gemv_w4p.hip: the binding table of the packed MXFP4 copies (mxfp4_bind.h), for the decode steps of model.hip: the binding
//      srgpt_mxfp4_bind made for the code array at W4, if it has exactly this shape ----
struct Mxfp4Binding;
bool srgpt_mxfp4_lookup(const void* W4, int N, int K, int swiglu, Mxfp4Binding* out);

// ---- attn.hip: the decode attention with the L2 prefetch of the next GEMV's weights, and its arrival tickets, for model.hip ----
int srgpt_decode_attention_pf(const void* qkv, void* kcache, void* vcache, const int* pos, const void* cos_tab,
                              const void* sin_tab, void* out, float* ws, int B, int Hq, int Hkv, int D, int max_pos, int dtype,
                              const void* next_w, int next_n, int next_k, int next_fp8, srgpt_stream_t stream);
void* srgpt_decode_attn_sync_words(float* ws, int B, int Hq, int D, size_t* bytes);

// the arrival tickets of srgpt_decode_attention_multi's workspace (srgpt_llm_lookup_sync_state reads them back)
void* srgpt_decode_attn_multi_sync_words(float* ws, int B, int T, int Hq, int D, size_t* bytes);

// ---- lookup.hip, for the lookup step of model.hip: the draft launch with the step's extras (tok / row_ids: the T ids the step
//      embeds, err: the state's sticky error word; all three NULL for the stand-alone entry) and the accept launch (picks NULL: the
//      rows' picks are merged from the PICK_SLICES partials pv / pi of argmax_partial_kernel) ----
int srgpt_lookup_rows_max();   // T = K + 1 rows a step can carry
int srgpt_lookup_ngram_max();  // ids of the trailing n-gram the matcher compares
int srgpt_lookup_draft_launch(const int64_t* prompt_ids, int n_prompt, const int64_t* out_ids, const int* step, int max_new, int K,
                              int max_ngram, int64_t vocab, int64_t* draft, int* n_draft, const int64_t* tok, int64_t* row_ids, int* err,
                              hipStream_t s);
int srgpt_lookup_accept_launch(const int64_t* picks, const float* pv, const int* pi, const int64_t* draft, const int* n_draft, int T,
                               int64_t* tok, int64_t* out_ids, int* pos, int* step, int max_new, int max_pos, int64_t* tok_emb, int* stats,
                               hipStream_t s);
// the accept of a SAMPLED step: the rows' picks were drawn by a rows-are-steps sampler launch below -- int64 ids in `drawn` (the
// top-k-64 sampler, select_drew, while sp->top_k >= 1) or PICK_SLICES partials per row in pv / pi; sp->counter += the ids emitted
int srgpt_lookup_accept_sampled_launch(srgpt_sampling* sp, int select_drew, const int64_t* drawn, const float* pv, const int* pi,
                                       const int64_t* draft, const int* n_draft, int T, int64_t* tok, int64_t* out_ids, int* pos, int* step,
                                       int max_new, int max_pos, int64_t* tok_emb, int* stats, hipStream_t s);
// the batched step's pair: B sequences of T = K + 1 rows, every sequence over its own history (prompt_ids [B, ld_prompt], n_prompt [B],
// steps [B] on the device); draft [B, K], n_draft [B], row_ids [B, T]; the accept also leaves *step = min over b of steps[b]
int srgpt_lookup_draft_batch_launch(const int64_t* prompt_ids, int ld_prompt, const int* n_prompt, const int64_t* out_ids, const int* steps,
                                    int B, int max_new, int K, int max_ngram, int64_t vocab, int64_t* draft, int* n_draft,
                                    const int64_t* tok, int64_t* row_ids, int* err, hipStream_t s);
int srgpt_lookup_accept_batch_launch(const int64_t* picks, const float* pv, const int* pi, const int64_t* draft, const int* n_draft, int B,
                                     int T, int64_t* tok, int64_t* out_ids, int* pos, int* steps, int* step, int max_new, int max_pos,
                                     int64_t* tok_emb, int* stats, hipStream_t s);
// the accept of a SAMPLED batched step: the B * T rows' picks were drawn by a B-sequences-x-T-steps sampler launch below (where they
// lie: as for srgpt_lookup_accept_sampled_launch); sp->counter += the columns of out_ids that filled up (draw_addr.h)
int srgpt_lookup_accept_batch_sampled_launch(srgpt_sampling* sp, int select_drew, const int64_t* drawn, const float* pv, const int* pi,
                                             const int64_t* draft, const int* n_draft, int B, int T, int64_t* tok, int64_t* out_ids,
                                             int* pos, int* steps, int* step, int max_new, int max_pos, int64_t* tok_emb, int* stats,
                                             hipStream_t s);

// ---- sample.hip, for greedy_pick of model.hip: the samplers' launches without the bookkeeping (slices, partials, workspaces: pick.h) ----
int srgpt_sample_launch(const float* logits, const srgpt_sampling* sp, int64_t* tok, void* ws, float* pv, int* pi, int* err, int B, int V,
                        hipStream_t s);
int srgpt_sample_full_launch(const float* logits, const srgpt_sampling* sp, void* keys_thr, float* pv, int* pi, unsigned* kept_mask, int B,
                             int V, hipStream_t s);
// ... and for the sampled lookup step: the same launches over T rows that are successive steps of ONE sequence (row t draws at
// Philox counter sp->counter + t, sequence 0: pick_draw, pick.h)
int srgpt_sample_rows_launch(const float* logits, const srgpt_sampling* sp, int64_t* tok, void* ws, float* pv, int* pi, int* err, int T,
                             int V, hipStream_t s);
int srgpt_sample_full_rows_launch(const float* logits, const srgpt_sampling* sp, void* keys_thr, float* pv, int* pi, unsigned* kept_mask,
                                  int T, int V, hipStream_t s);
// ... and for the batched sampled lookup step: over the B * T rows of B sequences x T successive steps (row b * T + t draws at
// draw_addr.h's address over the device counts steps [B]); pv / pi / tok / kept_mask hold B * T rows, the workspaces are sized for them
int srgpt_sample_seq_rows_launch(const float* logits, const srgpt_sampling* sp, const int* steps, int64_t* tok, void* ws, float* pv, int* pi,
                                 int* err, int B, int T, int V, hipStream_t s);
int srgpt_sample_full_seq_rows_launch(const float* logits, const srgpt_sampling* sp, const int* steps, void* keys_thr, float* pv, int* pi,
                                      unsigned* kept_mask, int B, int T, int V, hipStream_t s);

// ---- logits_proc.hip, for greedy_pick of model.hip: the logits processors' launch (n_dev != NULL: the history length on the device) ----
int srgpt_logits_proc_launch(float* scores, const srgpt_logits_proc* lp, const int64_t* ids, int ld, int n, const int* n_dev, int B, int V,
                             hipStream_t s);
int srgpt_logits_proc_max_history();  // ids per row the kernel can hold

// ---- flash.hip: the MFMA flash attention kernel's arguments and launcher, for srgpt_attention (attn.hip) ----
struct AttnArgs {
  const bf16_t *q, *k, *v;
  bf16_t* o;
  int Tq, Tk, Hq, Hkv, D;
  int64_t q_bs, q_ts, q_hs, k_bs, k_ts, k_hs, v_bs, v_ts, v_hs;
  float scale;
  const int* kv_len;
  const int* q_pos0;  // srgpt_attention_append: the causal offset of row b is q_pos0[b]; NULL (srgpt_attention): Tk - Tq
};
int srgpt_flash_bf16_launch(const AttnArgs& a, const AttnPrefillRoute& r, bool causal, hipStream_t s);
