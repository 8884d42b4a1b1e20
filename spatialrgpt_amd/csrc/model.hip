// Host-side composites over the per-op C ABI: vision tower forward, Llama prefill, device-side greedy
// decode step and its hipGraph.  Pure launch sequencing in C++ so one request costs a handful of
// FFI crossings instead of ~10^4 (SURVEY 3.1 hot loops); all state lives in caller-owned buffers.
#include <vector>

#include "attn_route.h"
#include "common.h"
#include "gemv_route.h"
#include "internal.h"
#include "mxfp4_bind.h"
#include "pack13_bind.h"
#include "pick.h"

namespace {

inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

struct Carver {
  char* base;
  size_t off = 0;
  explicit Carver(void* p) : base(reinterpret_cast<char*>(p)) {}
  void* take(size_t bytes) {
    void* r = base ? base + off : nullptr;
    off += align256(bytes);
    return r;
  }
};

// ---- ViT workspace ----
struct VitWs {
  void *col, *h, *qkv, *mlp, *gws;
  size_t gws_bytes, total;
};
VitWs carve_vit(const srgpt_vit_weights* w, int n_img, void* ws) {
  const size_t es = dtype_size(w->dtype);
  const int g = w->image_size / w->patch;
  const size_t rows = (size_t)n_img * (g * g + (w->cls_emb ? 1 : 0));
  Carver c(ws);
  VitWs v;
  v.col = c.take(rows * w->kp * es);
  v.h = c.take(rows * w->hidden * es);
  v.qkv = c.take(rows * 3 * w->hidden * es);
  v.mlp = c.take(rows * w->inter_pad * es);
  v.gws_bytes = (size_t)srgpt_gemm_ws_bytes((int)rows, w->hidden);  // split-K only pays on the narrow (N = hidden) GEMMs
  v.gws = c.take(v.gws_bytes);
  v.total = c.off;
  return v;
}

// ---- LLM workspace ----
struct LlmWs {
  void *x, *h, *qkv, *attn, *gu, *act, *last;  // prefill
  void *xd, *qkvd, *attnd, *actd;              // decode
  float* dws;
  void* gws;  // split-K workspace of the prefill GEMMs
  size_t gws_bytes;
  float* amax_v;  // [batch, PICK_SLICES] the pick's per-slice values (pick.h)
  int* amax_i;    // [batch, PICK_SLICES] their indices
  int64_t* tok_emb;  // [batch] the token whose embedding row currently sits in xd (-1: none)
  void* smp;         // sampling: the slices' top-k candidates (SampleWs, pick.h)
  void* smpf;        // full sampler: the row's keys and threshold pair (the head of SampleFullWs)
  int* err;          // sticky error word of the decode step (bit 0: a caller-written st->tok outside the table), read by srgpt_llm_decode_sync_state
  float* rowss;   // decode, 2+ rows: two row-statistics tables [batch][SRGPT_ROWSS_STRIDE] (o_proj's and down_proj's output rows)
  void* a8;       // fp8_act (W8A8 and W4A8 prefill): the e4m3 bytes of the current GEMM input [rows, max K]
  float* a8s;     // fp8_act: their per-row scales [rows]
  // srgpt_llm_prefill_append: [batch] the validated position every row's segment starts at, and [batch] that + the rows it appends
  // (the keys the row may see, its pos after the call).  They LIVE IN qkvd: the decode step's q/k/v scratch is dead between steps
  // (every step writes it before reading it) and holds >= 12 bytes per row, so the workspace does not grow
  int *app_pos0, *app_kvlen;
  void* w4;  // MXFP4 weights, bf16 activations: the bf16 expansion of the matrix the prefill multiplies next (sized for the largest
             // of the four); NULL with fp8_act (W4A8: nothing expands)
  size_t total;
};
LlmWs carve_llm(const srgpt_llm_weights* w, int batch, int max_tokens, void* ws) {
  const size_t es = dtype_size(w->dtype);
  const size_t rows = (size_t)batch * max_tokens;
  const size_t qkvw = (size_t)(w->heads + 2 * w->kv_heads) * w->head_dim;
  Carver c(ws);
  LlmWs l;
  l.x = c.take(rows * w->hidden * es);
  l.h = c.take(rows * w->hidden * es);
  l.qkv = c.take(rows * qkvw * es);
  l.attn = c.take(rows * (size_t)w->heads * w->head_dim * es);
  l.gu = c.take(rows * 2 * (size_t)w->inter * es);
  l.act = c.take(rows * (size_t)w->inter * es);
  l.last = c.take((size_t)batch * w->hidden * es);
  l.xd = c.take((size_t)batch * w->hidden * es);
  l.qkvd = c.take((size_t)batch * qkvw * es);
  l.attnd = c.take((size_t)batch * w->heads * w->head_dim * es);
  l.actd = c.take((size_t)batch * w->inter * es);
  l.dws = reinterpret_cast<float*>(c.take((size_t)srgpt_decode_attn_ws_floats(batch, w->heads, w->head_dim) * 4));
  l.gws_bytes = (size_t)srgpt_gemm_ws_bytes((int)rows, (int)(qkvw > (size_t)w->hidden ? qkvw : (size_t)w->hidden));
  l.gws = c.take(l.gws_bytes);
  l.amax_v = reinterpret_cast<float*>(c.take((size_t)batch * PICK_SLICES * 4));
  l.amax_i = reinterpret_cast<int*>(c.take((size_t)batch * PICK_SLICES * 4));
  l.tok_emb = reinterpret_cast<int64_t*>(c.take((size_t)batch * 8));
  l.err = reinterpret_cast<int*>(c.take(sizeof(int)));
  l.smp = c.take((size_t)carve_sample_ws(nullptr, batch).bytes);
  l.smpf = c.take(carve_sample_full_ws(nullptr, batch, w->vocab).head_bytes);
  l.rowss = reinterpret_cast<float*>(c.take((size_t)2 * batch * SRGPT_ROWSS_STRIDE * sizeof(float)));
  l.a8 = nullptr;
  l.a8s = nullptr;
  if (w->fp8_act) {
    size_t kmax = (size_t)w->hidden;
    if ((size_t)w->inter > kmax) kmax = (size_t)w->inter;
    if ((size_t)w->heads * w->head_dim > kmax) kmax = (size_t)w->heads * w->head_dim;
    l.a8 = c.take(rows * kmax);
    l.a8s = reinterpret_cast<float*>(c.take(rows * 4));
  }
  static_assert(sizeof(int) == 4, "two ints per row must fit the 12 bytes a row of qkvd has at least");
  l.app_pos0 = reinterpret_cast<int*>(l.qkvd);
  l.app_kvlen = l.qkvd ? l.app_pos0 + batch : nullptr;
  l.w4 = nullptr;
  if (w->wqkv4 && !w->fp8_act) {  // last: the layout of every other format is untouched
    const size_t hqd = (size_t)w->heads * w->head_dim;
    size_t n = qkvw * w->hidden;
    if (hqd * w->hidden > n) n = hqd * w->hidden;
    if (2 * (size_t)w->inter * w->hidden > n) n = 2 * (size_t)w->inter * w->hidden;
    l.w4 = c.take(n * 2);
  }
  l.total = c.off;
  return l;
}

__global__ void set_int_kernel(int* p, int n, int v) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) p[i] = v;
}

// srgpt_llm_prefill_append, first launch: every row's live length and segment length are DEVICE values the host only bounds
// (h_pos_max, T).  A row outside 0 <= pos <= h_pos_max or 1 <= len <= T raises bit 8 of the state's sticky error word and gets the
// nearest position / length that keeps every later write of the call inside the cache: pos0 in [0, max_pos - T], so rows
// pos0 .. pos0 + T - 1 exist whatever pos held.  (The host has checked h_pos_max + T <= max_pos: a valid row is never moved.)
constexpr int ERR_APPEND_ROW = 8;
__global__ void append_begin_kernel(const int* __restrict__ pos, const int* __restrict__ lens, int B, int T, int h_pos_max, int max_pos,
                                    int* __restrict__ pos0, int* __restrict__ kvlen, int* __restrict__ err) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const int p = pos[b], n = lens ? lens[b] : T;
  if (p < 0 || p > h_pos_max || n < 1 || n > T) atomicOr(err, ERR_APPEND_ROW);
  const int p0 = min(max(p, 0), max_pos - T), n0 = min(max(n, 1), T);
  pos0[b] = p0;
  kvlen[b] = p0 + n0;
}

// ... and its last but one: out[b, :] = x[b, len - 1, :] (16-byte chunks), len = kvlen[b] - pos0[b], and pos[b] = kvlen[b]
__global__ void append_end_kernel(const unsigned char* __restrict__ x, const int* __restrict__ pos0, const int* __restrict__ kvlen,
                                  unsigned char* __restrict__ out, int* __restrict__ pos, int T, int row_bytes) {
  const int b = blockIdx.x;
  const int len = kvlen[b] - pos0[b];
  const u32x4* src = reinterpret_cast<const u32x4*>(x + ((size_t)b * T + (len - 1)) * row_bytes);
  u32x4* dst = reinterpret_cast<u32x4*>(out + (size_t)b * row_bytes);
  for (int c = threadIdx.x; c < (row_bytes >> 4); c += blockDim.x) dst[c] = src[c];
  if (threadIdx.x == 0) pos[b] = kvlen[b];
}

// greedy pick, stage 1: each block scans a contiguous slice of one row (first max wins, like torch.argmax)
__global__ __launch_bounds__(256) void argmax_partial_kernel(const float* __restrict__ logits, float* __restrict__ pv,
                                                             int* __restrict__ pi, int V) {
  const PickSlice sl = pick_slice(V);
  const float* row = logits + (size_t)blockIdx.y * V;
  float best = -INFINITY;
  int bi = PICK_NONE;
  for (int i = sl.lo + threadIdx.x; i < sl.hi; i += 256) {
    const float v = row[i];
    if (v > best) {  // ascending scan per thread: the first maximum is kept
      best = v;
      bi = i;
    }
  }
  pick_store_slice(best, bi, pv, pi);
}

// stage 2 + bookkeeping: one wave per batch row merges the partials -> tok / out_ids[:, step] / pos / step, and (embed != NULL)
// the embedding rows of the picked tokens go straight into the residual-stream buffer of the next step (one launch fewer per token)
constexpr int ADVANCE_MAXB = 256;
__global__ __launch_bounds__(1024) void advance_kernel(const float* __restrict__ pv, const int* __restrict__ pi, int nb, int64_t* tok,
                               int64_t* out_ids, int* pos, int* step, int B, int max_new, int bump_pos,
                               const unsigned char* __restrict__ embed, unsigned char* __restrict__ xd, int row_bytes,
                               int64_t* __restrict__ tok_emb, srgpt_sampling* __restrict__ sp, int select_drew) {
  __shared__ int picked[ADVANCE_MAXB];
  const int s = *step;
  const int lane = threadIdx.x & 63;
  // sampling with a top-k filter: sample_select_kernel already drew tok[b]; greedy, Gumbel-max sampling (top_k = 0) and the full
  // sampler (select_drew = 0): the slices' maxima are merged here
  const bool drawn = sp != nullptr && select_drew && sp->top_k > 0;
  for (int b = threadIdx.x >> 6; b < B; b += blockDim.x >> 6) {
    const int64_t t = drawn ? tok[b] : pick_merge_row(pv + (size_t)b * nb, pi + (size_t)b * nb, nb, lane);
    if (lane == 0) {
      tok[b] = t;
      if (embed && b < ADVANCE_MAXB) {
        picked[b] = (int)t;
        tok_emb[b] = t;  // the row written below belongs to this token (embed_sync_kernel checks it)
      }
      if (s < max_new) out_ids[(size_t)b * max_new + s] = t;
      if (bump_pos) pos[b] += 1;
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    *step = s + 1;
    if (sp) sp->counter += 1;  // the next step draws from a fresh Philox counter
  }
  if (embed) {
    // the rows of the picked tokens, four independent 16-byte loads in flight per thread (one at a time, a dependent load -> store
    // chain per chunk, this copy was 8 of the kernel's 13 us at 8 sequences)
    const int per_row = row_bytes >> 4;  // 16-byte chunks per embedding row
    const int total = B * per_row, nt = blockDim.x;
    for (int i0 = threadIdx.x; i0 < total; i0 += 4 * nt) {
      u32x4 v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int i = min(i0 + u * nt, total - 1);
        const int b = i / per_row, c = i - b * per_row;
        v[u] = *reinterpret_cast<const u32x4*>(embed + (size_t)picked[b] * row_bytes + (size_t)c * 16);
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int i = i0 + u * nt;
        if (i < total) {
          const int b = i / per_row, c = i - b * per_row;
          *reinterpret_cast<u32x4*>(xd + (size_t)b * row_bytes + (size_t)c * 16) = v[u];
        }
      }
    }
  }
}

// First node of the CAPTURED decode step: xd must hold the embedding rows of st->tok.  Normally advance_kernel of the step before
// left exactly those rows (tok_emb == tok: B compares, nothing copied); a caller that wrote its own token into st->tok between
// replays -- valid under ABI 1/2, silently ignored in ABI 3 -- gets its row re-embedded here.  A caller-written id
// outside the table cannot be embedded: the step would run on the previous token's row and return plausible ids, so it sets a
// sticky error bit that srgpt_llm_decode_sync_state reports.
__global__ void embed_sync_kernel(const int64_t* __restrict__ tok, int64_t* __restrict__ tok_emb,
                                  const unsigned char* __restrict__ embed, unsigned char* __restrict__ xd, int B, int row_bytes,
                                  int64_t vocab, int* __restrict__ err) {
  const int per_row = row_bytes >> 4;
  for (int b = blockIdx.x; b < B; b += gridDim.x) {
    const int64_t t = tok[b];
    if (t == tok_emb[b]) continue;  // uniform per block
    if (t < 0 || t >= vocab) {
      if (threadIdx.x == 0) atomicOr(err, 1);
      continue;
    }
    for (int c = threadIdx.x; c < per_row; c += blockDim.x)
      *reinterpret_cast<u32x4*>(xd + (size_t)b * row_bytes + (size_t)c * 16) =
          *reinterpret_cast<const u32x4*>(embed + (size_t)t * row_bytes + (size_t)c * 16);
    __syncthreads();
    if (threadIdx.x == 0) tok_emb[b] = t;
  }
}

// the eager step embeds st->tok itself (srgpt_embed_rows): record whose rows are in place, so that the invariant "xd holds the
// rows of tok_emb" does not depend on a greedy_pick always following
__global__ void record_embedded_kernel(const int64_t* __restrict__ tok, int64_t* __restrict__ tok_emb, int B) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b < B) tok_emb[b] = tok[b];
}

// the next step's embedding rows can come from advance_kernel when they are whole 16-byte chunks and the batch fits its LDS list
static inline bool advance_embeds(const srgpt_llm_weights* w, const srgpt_llm_state* st) {
  return st->batch <= ADVANCE_MAXB && ((size_t)w->hidden * dtype_size(w->dtype)) % 16 == 0;
}

// how a step picks: the sampler kind that draws while st->sampling is set (SRGPT_SAMPLER_*), and the logits processors' block
// (NULL: none) -- what the plain, _ex and _proc forms of an entry point differ in
struct Pick {
  int sampler;
  const srgpt_logits_proc* lp;
};

// the next token of every sequence from st->logits: argmax (st->sampling == NULL) or a draw by the sampler p.sampler (sample.hip),
// then the bookkeeping.  p.lp != NULL: the logits processors (logits_proc.hip) rewrite st->logits first, over the ids generated so
// far (st->out_ids, *st->step of them).  Every producer leaves PICK_SLICES pairs per row (pick.h) for advance_kernel's merge
static int greedy_pick(const srgpt_llm_weights* w, srgpt_llm_state* st, const LlmWs& d, int bump_pos, Pick p, hipStream_t s) {
  const int B = st->batch;
  const bool emb = advance_embeds(w, st);
  if (p.lp) SRGPT_TRY(srgpt_logits_proc_launch(st->logits, p.lp, st->out_ids, st->max_new, 0, st->step, B, w->vocab, s));
  if (st->sampling) {
    if (p.sampler == SRGPT_SAMPLER_FULL)
      SRGPT_TRY(srgpt_sample_full_launch(st->logits, st->sampling, d.smpf, d.amax_v, d.amax_i, nullptr, B, w->vocab, s));
    else
      SRGPT_TRY(srgpt_sample_launch(st->logits, st->sampling, st->tok, d.smp, d.amax_v, d.amax_i, d.err, B, w->vocab, s));
  } else {
    hipLaunchKernelGGL(argmax_partial_kernel, dim3(PICK_SLICES, B), dim3(256), 0, s, st->logits, d.amax_v, d.amax_i, w->vocab);
  }
  hipLaunchKernelGGL(advance_kernel, dim3(1), dim3(B > 4 ? 1024 : 256), 0, s, d.amax_v, d.amax_i, PICK_SLICES, st->tok, st->out_ids,
                     st->pos, st->step, B, st->max_new, bump_pos, emb ? reinterpret_cast<const unsigned char*>(w->embed) : nullptr,
                     reinterpret_cast<unsigned char*>(d.xd), (int)((size_t)w->hidden * dtype_size(w->dtype)), d.tok_emb, st->sampling,
                     p.sampler == SRGPT_SAMPLER_TOPK64 ? 1 : 0);
  SRGPT_LAUNCH_CHECK();
  return SRGPT_OK;
}

}  // namespace

struct srgpt_graph {
  hipGraph_t graph;
  hipGraphExec_t exec;
};

// ================================================================================================
// vision tower
// ================================================================================================
extern "C" int64_t srgpt_vit_ws_bytes(const srgpt_vit_weights* w, int n_img) {
  if (!w || n_img <= 0) return -1;
  return (int64_t)carve_vit(w, n_img, nullptr).total;
}

extern "C" int srgpt_vit_forward(const srgpt_vit_weights* w, const void* images, void* out, void* ws, int n_img,
                                 srgpt_stream_t stream) {
  SRGPT_CHECK(w && images && out && ws && n_img > 0, SRGPT_ERR_ARG, "srgpt_vit_forward: bad args");
  // image_size need not be a multiple of patch: a 'valid' conv drops the remainder (384 px / 14 -> 27 patches)
  SRGPT_CHECK(w->hidden % w->heads == 0 && w->image_size >= w->patch, SRGPT_ERR_ARG, "srgpt_vit_forward: bad config");
  SRGPT_CHECK(w->inter_pad >= w->inter && w->inter_pad % 8 == 0, SRGPT_ERR_ARG, "srgpt_vit_forward: inter_pad %d < inter %d",
              w->inter_pad, w->inter);
  const int dt = w->dtype, C = w->hidden, I = w->inter, IP = w->inter_pad, H = w->heads, hd = C / H;
  const int g = w->image_size / w->patch, gg = g * g, L = gg + (w->cls_emb ? 1 : 0), rows = n_img * L;
  const VitWs v = carve_vit(w, n_img, ws);
  void* x = out;  // residual stream lives in the output buffer
  SRGPT_TRY(srgpt_im2col(images, v.col, n_img, w->image_size, w->patch, w->kp, dt, stream));
  if (!w->cls_emb) {
    // SigLIP: conv-as-GEMM + bias, then + position embedding (row m uses pos_emb[m % L])
    SRGPT_TRY(srgpt_gemm(v.col, w->patch_w, w->patch_b, w->pos_emb, x, rows, C, w->kp, w->kp, C, SRGPT_ACT_NONE, 0, L, 0,
                         SRGPT_OUT_PLAIN, 0, v.gws, (int64_t)v.gws_bytes, dt, stream));
  } else {
    // CLIP: patch GEMM (no bias) -> [cls | patches] + position embedding -> pre_layrnorm
    SRGPT_TRY(srgpt_gemm(v.col, w->patch_w, w->patch_b, nullptr, v.h, n_img * gg, C, w->kp, w->kp, C, SRGPT_ACT_NONE, 0, 0, 0,
                         SRGPT_OUT_PLAIN, 0, v.gws, (int64_t)v.gws_bytes, dt, stream));
    SRGPT_TRY(srgpt_vit_assemble_cls(v.h, w->cls_emb, w->pos_emb, x, n_img, gg, C, dt, stream));
    if (w->pre_ln_w) SRGPT_TRY(srgpt_layernorm(x, w->pre_ln_w, w->pre_ln_b, x, rows, C, w->eps, SRGPT_ACT_NONE, dt, stream));
  }
  const float scale = 1.0f / sqrtf((float)hd);
  const char* qkv = reinterpret_cast<const char*>(v.qkv);
  const size_t es = dtype_size(dt);
  if (IP > I)  // the pad columns of the MLP activation buffer: zero once per forward (fc1 never writes them, w2 is zero there)
    SRGPT_HIP_TRY(hipMemset2DAsync(reinterpret_cast<char*>(v.mlp) + (size_t)I * es, (size_t)IP * es, 0, (size_t)(IP - I) * es,
                                   (size_t)rows, as_stream(stream)),
                  "srgpt_vit_forward: zeroing the activation pad");
  // The LayerNorm that follows out_proj / fc2 rides in the product's split-K reduction when there is one (srgpt_gemm_norm: bit-identical
  // to the two launches); ln1 of the first layer is the only stand-alone norm.
  for (int l = 0; l < w->n_layers_run; ++l) {
    if (l == 0) SRGPT_TRY(srgpt_layernorm(x, w->ln1_w[l], w->ln1_b[l], v.h, rows, C, w->eps, SRGPT_ACT_NONE, dt, stream));
    SRGPT_TRY(srgpt_gemm(v.h, w->wqkv[l], w->bqkv[l], nullptr, v.qkv, rows, 3 * C, C, C, 3 * C, SRGPT_ACT_NONE, 0, 0, 0,
                         SRGPT_OUT_PLAIN, 0, v.gws, (int64_t)v.gws_bytes, dt, stream));
    SRGPT_TRY(srgpt_attention(qkv, qkv + (size_t)C * es, qkv + (size_t)2 * C * es, v.h, n_img, L, L, H, H, hd,
                              (int64_t)L * 3 * C, 3 * C, hd, (int64_t)L * 3 * C, 3 * C, hd, (int64_t)L * 3 * C, 3 * C, hd,
                              scale, 0, nullptr, dt, stream));
    SRGPT_TRY(srgpt_gemm_norm(v.h, w->wo[l], w->bo[l], x, x, rows, C, C, v.gws, (int64_t)v.gws_bytes, SRGPT_NORM_LAYER, w->ln2_w[l],
                              w->ln2_b[l], v.h, w->eps, dt, stream));
    SRGPT_TRY(srgpt_gemm(v.h, w->w1[l], w->b1[l], nullptr, v.mlp, rows, I, C, C, IP, w->act, 0, 0, 0,
                         SRGPT_OUT_PLAIN, 0, v.gws, (int64_t)v.gws_bytes, dt, stream));
    if (l + 1 < w->n_layers_run)
      SRGPT_TRY(srgpt_gemm_norm(v.mlp, w->w2[l], w->b2[l], x, x, rows, C, IP, v.gws, (int64_t)v.gws_bytes, SRGPT_NORM_LAYER,
                                w->ln1_w[l + 1], w->ln1_b[l + 1], v.h, w->eps, dt, stream));
    else
      SRGPT_TRY(srgpt_gemm(v.mlp, w->w2[l], w->b2[l], x, x, rows, C, IP, IP, C, SRGPT_ACT_NONE, 0, 0, 0, SRGPT_OUT_PLAIN, 0, v.gws,
                           (int64_t)v.gws_bytes, dt, stream));
  }
  return SRGPT_OK;
}

// ================================================================================================
// Llama decoder
// ================================================================================================
extern "C" int64_t srgpt_llm_ws_bytes(const srgpt_llm_weights* w, int batch, int max_tokens) {
  if (!w || batch <= 0 || max_tokens <= 0) return -1;
  return (int64_t)carve_llm(w, batch, max_tokens, nullptr).total;
}

static int check_llm(const srgpt_llm_weights* w, const srgpt_llm_state* st) {
  SRGPT_CHECK(w && st, SRGPT_ERR_ARG, "llm: null weights/state");
  SRGPT_CHECK(st->kcache && st->vcache && st->pos && st->tok && st->out_ids && st->step && st->ws && st->logits,
              SRGPT_ERR_ARG, "llm: state has null buffers");
  SRGPT_CHECK(w->heads % w->kv_heads == 0 && w->head_dim % 2 == 0, SRGPT_ERR_ARG, "llm: bad head config");
  SRGPT_CHECK(st->batch > 0 && st->max_pos > 0 && st->ws_tokens > 0 && st->max_new > 0, SRGPT_ERR_ARG, "llm: bad state sizes");
  return SRGPT_OK;
}

// out[b, :] = x[b, lens[b] - 1, :] (16-byte chunks) and pos[b] = lens[b]
template <typename T>
__global__ void gather_last_rows_kernel(const T* __restrict__ x, const int* __restrict__ lens, T* __restrict__ out,
                                        int* __restrict__ pos, int Tlen, int Hd) {
  const int b = blockIdx.x;
  const int len = min(max(lens[b], 1), Tlen);
  constexpr int VEC = Vec16<T>::N;
  const Vec16<T>* src = reinterpret_cast<const Vec16<T>*>(x + ((size_t)b * Tlen + (len - 1)) * Hd);
  Vec16<T>* dst = reinterpret_cast<Vec16<T>*>(out + (size_t)b * Hd);
  for (int c = threadIdx.x; c < Hd / VEC; c += blockDim.x) dst[c] = src[c];
  if (threadIdx.x == 0) pos[b] = len;
}

namespace {

// ---- weight formats ----
// FMT_DTYPE: the dtype matrices (srgpt_gemm / srgpt_gemv).  fp8 copies present -> they are the weights and the dtype matrices are
// not touched: FMT_W8A16 (srgpt_gemm_w8 / srgpt_gemv_w8; the decode step streams half the bytes per token), or with fp8_act
// FMT_W8A8: the prefill's per-token e4m3 activations on the fp8 matrix pipe (include/srgpt.h).  The decode step and the
// all-position lm_head (fp32 logits, parity hook) are W8A16 under both fp8 formats.  MXFP4 copies present -> FMT_W4A16: the four
// layer matrices are codes + block scales (srgpt_gemv_w4 in the decode steps, the srgpt_gemm_w4 family in the prefill), lm_head
// is fp8 and multiplied as under FMT_W8A16.  FMT_W4A8 (MXFP4 copies and fp8_act) exists in prefill_impl only: the prefill's products
// are srgpt_gemm_w4a8 on per-token e4m3 activations; llm_format() reports FMT_W4A16 for such weights and every step entry runs that.
enum LlmFormat { FMT_DTYPE, FMT_W8A16, FMT_W8A8, FMT_W4A16, FMT_W4A8 };

// the format of `w` and the check that fp8 weights are complete, on the host before any launch; `fn`: the entry point the message names
int llm_format(const srgpt_llm_weights* w, const char* fn, LlmFormat* fmt) {
  *fmt = FMT_DTYPE;
  SRGPT_CHECK(w->decode_pass_rows == 0 || w->decode_pass_rows == 16 || w->decode_pass_rows == GEMV_WIDE_ROWS, SRGPT_ERR_ARG,
              "%s: decode_pass_rows = %d (0 or 16: passes of 16 rows; %d: the wide pass)", fn, w->decode_pass_rows, GEMV_WIDE_ROWS);
  SRGPT_CHECK(w->mxfp4_direct == 0 || (w->mxfp4_direct == 1 && w->wqkv4), SRGPT_ERR_ARG,
              "%s: mxfp4_direct = %d (0: the plain W4 entries; 1: the _direct entries, MXFP4 weights only)", fn, w->mxfp4_direct);
  if (w->wqkv4) {
    SRGPT_CHECK(w->dtype == SRGPT_BF16 && w->wo4 && w->wgu4 && w->wdown4 && w->wqkv4_scale && w->wo4_scale && w->wgu4_scale &&
                    w->wdown4_scale && w->lm_head8 && w->lm_head_scale,
                SRGPT_ERR_ARG, "%s: MXFP4 weights need bf16 activations, all four matrices + block scales and the fp8 lm_head + scales", fn);
    SRGPT_CHECK(!w->wqkv8, SRGPT_ERR_ARG, "%s: both fp8 and MXFP4 copies of the layer matrices are set", fn);
    SRGPT_CHECK(w->hidden % 32 == 0 && w->inter % 32 == 0 && (w->heads * w->head_dim) % 32 == 0, SRGPT_ERR_ARG,
                "%s: MXFP4 weights need hidden, inter and heads * head_dim to be multiples of 32", fn);
    *fmt = FMT_W4A16;
    return SRGPT_OK;
  }
  if (!w->wqkv8) return SRGPT_OK;
  SRGPT_CHECK(w->dtype == SRGPT_BF16 && w->wo8 && w->wgu8 && w->wdown8 && w->lm_head8 && w->wqkv_scale && w->wo_scale &&
                  w->wgu_scale && w->wdown_scale && w->lm_head_scale,
              SRGPT_ERR_ARG, "%s: fp8 weights need bf16 activations and all five matrices + scales", fn);
  *fmt = w->fp8_act != 0 ? FMT_W8A8 : FMT_W8A16;
  return SRGPT_OK;
}

// one weight matrix in the forms the products take
struct Mat {
  const void* w;       // row-major, engine dtype
  const void* w8;      // row-major fp8 bytes (NULL under FMT_DTYPE)
  const float* scale;  // their row scales
  const void* pk;      // packed copy of the fp8 bytes for the MFMA decode kernel, or NULL: stream the row-major ones
  int pk_rows;         // its rows per granule
  const void* w4;      // MXFP4 codes (FMT_W4A16 / FMT_W4A8 only; then w / w8 are not read)
  const void* scale4;  // their E8M0 block scales
};
struct LayerMats {
  Mat qkv, o, gu, down;
};
LayerMats layer_mats(const srgpt_llm_weights* w, LlmFormat fmt, int i) {
  if (fmt == FMT_W4A16 || fmt == FMT_W4A8) {
    auto mat4 = [&](const void* const* W4, const void* const* sc4) { return Mat{nullptr, nullptr, nullptr, nullptr, 0, W4[i], sc4[i]}; };
    return LayerMats{mat4(w->wqkv4, w->wqkv4_scale), mat4(w->wo4, w->wo4_scale), mat4(w->wgu4, w->wgu4_scale),
                     mat4(w->wdown4, w->wdown4_scale)};
  }
  const bool fp8 = fmt != FMT_DTYPE;
  auto mat = [&](const void* const* W, const void* const* W8, const float* const* sc, const void* const* pk, int pk_rows) {
    return Mat{W[i], fp8 ? W8[i] : nullptr, fp8 ? sc[i] : nullptr, fp8 && pk != nullptr ? pk[i] : nullptr, pk_rows, nullptr, nullptr};
  };
  return LayerMats{mat(w->wqkv, w->wqkv8, w->wqkv_scale, w->wqkv8p, w->pk_rows_qkv), mat(w->wo, w->wo8, w->wo_scale, w->wo8p, w->pk_rows_o),
                   mat(w->wgu, w->wgu8, w->wgu_scale, w->wgu8p, w->pk_rows_gu),
                   mat(w->wdown, w->wdown8, w->wdown_scale, w->wdown8p, w->pk_rows_down)};
}
// lm_head has no packed and no MXFP4 copy: engine dtype, or fp8 under every other format
Mat lm_head_mat(const srgpt_llm_weights* w) { return Mat{w->lm_head, w->lm_head8, w->lm_head_scale, nullptr, 0, nullptr, nullptr}; }

// ---- prefill ----
// One prefill's shapes, workspace and stream; the launches its layers are made of; and, per weight format, the launch sequence of
// layer i in order (layer_*).  Everything the formats share is in prefill_impl.
struct Prefill {
  const srgpt_llm_weights* w;
  const srgpt_llm_state* st;
  LlmWs l;
  LlmFormat fmt;
  int B, T, rows, Hd, I, HqD, QW, dt;
  srgpt_stream_t stream;
  // srgpt_llm_prefill_append: the rows continue at pos0[b] (device, validated) and see the keys below kvlen[b], at most Tk of
  // them (the host's bound); NULL / NULL / T: a prefill, every row starts at position 0
  const int* pos0;
  const int* kvlen;
  int Tk;

  int64_t gws_bytes() const { return (int64_t)l.gws_bytes; }
  char* cache(void* base, int i) const {
    return reinterpret_cast<char*>(base) + (size_t)i * B * w->kv_heads * st->max_pos * w->head_dim * dtype_size(dt);
  }
  // l.h = RMSNorm(l.x)
  int norm(const void* norm_w) const { return srgpt_rmsnorm(l.x, norm_w, l.h, rows, Hd, w->rms_eps, dt, stream); }
  int rope_append(int i) const {
    return srgpt_rope_kv_append(l.qkv, cache(st->kcache, i), cache(st->vcache, i), pos0, w->rope_cos, w->rope_sin, B, T, w->heads,
                                w->kv_heads, w->head_dim, st->max_pos, dt, stream);
  }
  int attention(int i) const {
    const int Hkv = w->kv_heads, D = w->head_dim;
    if (pos0)
      return srgpt_attention_append(l.qkv, cache(st->kcache, i), cache(st->vcache, i), l.attn, B, T, Tk, w->heads, Hkv, D,
                                    (int64_t)T * QW, QW, D, (int64_t)Hkv * st->max_pos * D, D, (int64_t)st->max_pos * D,
                                    (int64_t)Hkv * st->max_pos * D, D, (int64_t)st->max_pos * D, 1.0f / sqrtf((float)D), pos0, kvlen, dt,
                                    stream);
    return srgpt_attention(l.qkv, cache(st->kcache, i), cache(st->vcache, i), l.attn, B, T, T, w->heads, Hkv, D, (int64_t)T * QW, QW, D,
                           (int64_t)Hkv * st->max_pos * D, D, (int64_t)st->max_pos * D, (int64_t)Hkv * st->max_pos * D, D,
                           (int64_t)st->max_pos * D, 1.0f / sqrtf((float)D), 1, nullptr, dt, stream);
  }
  // W8A16 product: out = a @ m^T (+ res)
  int gemm_w8(const void* a, const Mat& m, const void* res, void* out, int N, int K) const {
    return srgpt_gemm_w8(a, m.w8, m.scale, nullptr, res, out, rows, N, K, K, N, SRGPT_ACT_NONE, 0, l.gws, gws_bytes(), stream);
  }
  // W8A8 / W4A8: the rows of `a` -> e4m3 bytes + per-token scales (l.a8, l.a8s), and the product of the rows quantised last with the
  // format's weights (fp8 bytes + row scales, or MXFP4 codes + block scales)
  int quant(const void* a, int K) const { return srgpt_quant_rows_e4m3(a, l.a8, l.a8s, rows, K, K, stream); }
  int gemm_w8a8(const Mat& m, const void* res, void* out, int N, int K) const {
    if (fmt == FMT_W4A8)
      return srgpt_gemm_w4a8(l.a8, l.a8s, m.w4, m.scale4, nullptr, res, out, rows, N, K, K, N, 0, l.gws, gws_bytes(), stream);
    return srgpt_gemm_w8a8(l.a8, l.a8s, m.w8, m.scale, nullptr, res, out, rows, N, K, K, N, 0, l.gws, gws_bytes(), stream);
  }

  // dtype matrices: the RMSNorm that follows o_proj / down_proj rides in the product's split-K reduction (srgpt_gemm_norm:
  // bit-identical to the two launches, one launch and one pass over the rows less per norm), so only layer 0 normalises l.x itself
  int layer_dtype(int i) const {
    const LayerMats m = layer_mats(w, fmt, i);
    if (i == 0) SRGPT_TRY(norm(w->attn_norm[i]));
    // projection + RoPE + cache append: the rotation rides in the split-K reduction
    SRGPT_TRY(srgpt_gemm_rope_kv_append(l.h, m.qkv.w, l.qkv, Hd, l.gws, gws_bytes(), cache(st->kcache, i), cache(st->vcache, i), pos0,
                                        w->rope_cos, w->rope_sin, B, T, w->heads, w->kv_heads, w->head_dim, st->max_pos, dt, stream));
    SRGPT_TRY(attention(i));
    SRGPT_TRY(srgpt_gemm_norm(l.attn, m.o.w, nullptr, l.x, l.x, rows, Hd, HqD, l.gws, gws_bytes(), SRGPT_NORM_RMS, w->mlp_norm[i], nullptr,
                              l.h, w->rms_eps, dt, stream));
    // gate / up + SiLU * up: the activation is the product's epilogue on the whole-M kernel
    SRGPT_TRY(srgpt_gemm_swiglu(l.h, m.gu.w, l.act, rows, I, Hd, l.gu, l.gws, gws_bytes(), dt, stream));
    if (i + 1 < w->layers)
      return srgpt_gemm_norm(l.act, m.down.w, nullptr, l.x, l.x, rows, Hd, I, l.gws, gws_bytes(), SRGPT_NORM_RMS, w->attn_norm[i + 1],
                             nullptr, l.h, w->rms_eps, dt, stream);
    return srgpt_gemm(l.act, m.down.w, nullptr, l.x, l.x, rows, Hd, I, I, Hd, SRGPT_ACT_NONE, 0, 0, 0, SRGPT_OUT_PLAIN, 0, l.gws,
                      gws_bytes(), dt, stream);
  }

  // MXFP4 matrices: layer_dtype's sequence through the W4 entry points (include/srgpt.h), which take the route of the bf16 product and
  // return its bits on the dequantised matrix: every byte the prefill writes equals a bf16 engine's on the dequantised weights.  On the
  // direct-to-LDS kernels (every product of an append, o_proj of the bs = 1 prefill) the codes are multiplied in the kernel; the
  // whole-M and 256 x 256 routes still expand each matrix (srgpt_dequant_mxfp4, exact) into the workspace's one bf16 scratch l.w4
  // just before its product -- the stream orders product -> next expansion, so one scratch serves the four.
  // srgpt_llm_weights::mxfp4_direct = 1: the same sequence through the `_direct` entries, where the whole-M kernel multiplies the
  // codes too (q/k/v, gate/up and down_proj of the 225 .. 272-row prefill); the scratch stays for the routes that still expand.
  int layer_w4a16(int i) const {
    const LayerMats m = layer_mats(w, fmt, i);
    const bool direct = w->mxfp4_direct == 1;
    const auto gemm_rope = direct ? srgpt_gemm_w4_rope_kv_append_direct : srgpt_gemm_w4_rope_kv_append;
    const auto gemm_norm = direct ? srgpt_gemm_w4_norm_direct : srgpt_gemm_w4_norm;
    const auto gemm_swiglu = direct ? srgpt_gemm_w4_swiglu_direct : srgpt_gemm_w4_swiglu;
    const auto gemm = direct ? srgpt_gemm_w4_direct : srgpt_gemm_w4;
    if (i == 0) SRGPT_TRY(norm(w->attn_norm[i]));
    SRGPT_TRY(gemm_rope(l.h, m.qkv.w4, m.qkv.scale4, l.qkv, Hd, l.w4, l.gws, gws_bytes(), cache(st->kcache, i), cache(st->vcache, i), pos0,
                        w->rope_cos, w->rope_sin, B, T, w->heads, w->kv_heads, w->head_dim, st->max_pos, stream));
    SRGPT_TRY(attention(i));
    SRGPT_TRY(gemm_norm(l.attn, m.o.w4, m.o.scale4, l.x, l.x, rows, Hd, HqD, l.w4, l.gws, gws_bytes(), w->mlp_norm[i], l.h, w->rms_eps,
                        stream));
    SRGPT_TRY(gemm_swiglu(l.h, m.gu.w4, m.gu.scale4, l.act, rows, I, Hd, l.gu, l.w4, l.gws, gws_bytes(), stream));
    if (i + 1 < w->layers)
      return gemm_norm(l.act, m.down.w4, m.down.scale4, l.x, l.x, rows, Hd, I, l.w4, l.gws, gws_bytes(), w->attn_norm[i + 1], l.h,
                       w->rms_eps, stream);
    return gemm(l.act, m.down.w4, m.down.scale4, l.x, l.x, rows, Hd, I, I, Hd, 0, l.w4, l.gws, gws_bytes(), stream);
  }

  int layer_w8a16(int i) const {
    const LayerMats m = layer_mats(w, fmt, i);
    SRGPT_TRY(norm(w->attn_norm[i]));
    SRGPT_TRY(gemm_w8(l.h, m.qkv, nullptr, l.qkv, QW, Hd));
    SRGPT_TRY(rope_append(i));
    SRGPT_TRY(attention(i));
    SRGPT_TRY(gemm_w8(l.attn, m.o, l.x, l.x, Hd, HqD));
    SRGPT_TRY(norm(w->mlp_norm[i]));
    SRGPT_TRY(gemm_w8(l.h, m.gu, nullptr, l.gu, 2 * I, Hd));
    SRGPT_TRY(srgpt_silu_mul(l.gu, l.act, rows, I, dt, stream));
    return gemm_w8(l.act, m.down, l.x, l.x, Hd, I);
  }

  // W8A8 and W4A8 (one sequence: gemm_w8a8 takes the format's weights), rows of up to 16384 columns: the producer of a GEMM's input rows (RMSNorm, SwiGLU) is fused into their per-token
  // quantisation -- the bf16 intermediate is neither written nor read (bit-identical to the two launches: tests/test_gpu_fp8_mfma.py)
  int layer_w8a8(int i) const {
    const LayerMats m = layer_mats(w, fmt, i);
    SRGPT_TRY(srgpt_quant_rows_e4m3_rmsnorm(l.x, w->attn_norm[i], w->rms_eps, l.a8, l.a8s, rows, Hd, Hd, stream));
    SRGPT_TRY(gemm_w8a8(m.qkv, nullptr, l.qkv, QW, Hd));
    SRGPT_TRY(rope_append(i));
    SRGPT_TRY(attention(i));
    SRGPT_TRY(quant(l.attn, HqD));
    SRGPT_TRY(gemm_w8a8(m.o, l.x, l.x, Hd, HqD));
    SRGPT_TRY(srgpt_quant_rows_e4m3_rmsnorm(l.x, w->mlp_norm[i], w->rms_eps, l.a8, l.a8s, rows, Hd, Hd, stream));
    SRGPT_TRY(gemm_w8a8(m.gu, nullptr, l.gu, 2 * I, Hd));
    SRGPT_TRY(srgpt_quant_rows_e4m3_swiglu(l.gu, l.a8, l.a8s, rows, I, stream));
    return gemm_w8a8(m.down, l.x, l.x, Hd, I);
  }

  // W8A8 and W4A8, wider rows (Llama-3-70B: inter 28672): the W8A16 sequence with every product's input quantised by a launch of its own
  int layer_w8a8_wide(int i) const {
    const LayerMats m = layer_mats(w, fmt, i);
    SRGPT_TRY(norm(w->attn_norm[i]));
    SRGPT_TRY(quant(l.h, Hd));
    SRGPT_TRY(gemm_w8a8(m.qkv, nullptr, l.qkv, QW, Hd));
    SRGPT_TRY(rope_append(i));
    SRGPT_TRY(attention(i));
    SRGPT_TRY(quant(l.attn, HqD));
    SRGPT_TRY(gemm_w8a8(m.o, l.x, l.x, Hd, HqD));
    SRGPT_TRY(norm(w->mlp_norm[i]));
    SRGPT_TRY(quant(l.h, Hd));
    SRGPT_TRY(gemm_w8a8(m.gu, nullptr, l.gu, 2 * I, Hd));
    SRGPT_TRY(srgpt_silu_mul(l.gu, l.act, rows, I, dt, stream));
    SRGPT_TRY(quant(l.act, I));
    return gemm_w8a8(m.down, l.x, l.x, Hd, I);
  }
};

}  // namespace

// h_pos_max < 0: a prefill (every row starts at position 0).  h_pos_max >= 0: srgpt_llm_prefill_append -- the rows continue at
// st->pos[b] <= h_pos_max, the same launches with the per-row positions in the RoPE / append and attention calls, one validation
// launch in front and without the prefill's re-arming of the decode tickets and the error word
static int prefill_impl(const srgpt_llm_weights* w, srgpt_llm_state* st, const void* inputs_embeds, int T, const int* lens,
                        int h_pos_max, float* all_logits, void* hidden_out, srgpt_stream_t stream) {
  const bool append = h_pos_max >= 0;
  SRGPT_TRY(check_llm(w, st));
  if (append) {
    SRGPT_CHECK(inputs_embeds, SRGPT_ERR_ARG, "srgpt_llm_prefill_append: inputs_embeds is null");
    SRGPT_CHECK(T > 0 && T <= st->ws_tokens, SRGPT_ERR_ARG, "srgpt_llm_prefill_append: T=%d outside 1 .. ws_tokens=%d", T, st->ws_tokens);
    SRGPT_CHECK((int64_t)h_pos_max + T <= st->max_pos, SRGPT_ERR_ARG,
                "srgpt_llm_prefill_append: h_pos_max=%d + T=%d exceeds max_pos=%d", h_pos_max, T, st->max_pos);
  } else {
    SRGPT_CHECK(inputs_embeds && T > 0 && T <= st->max_pos, SRGPT_ERR_ARG, "srgpt_llm_prefill: T=%d exceeds max_pos=%d", T,
                st->max_pos);
    SRGPT_CHECK(T <= st->ws_tokens, SRGPT_ERR_ARG, "srgpt_llm_prefill: T=%d exceeds ws_tokens=%d", T, st->ws_tokens);
  }
  LlmFormat fmt;
  SRGPT_TRY(llm_format(w, append ? "srgpt_llm_prefill_append" : "srgpt_llm_prefill", &fmt));
  const int dt = w->dtype, Hd = w->hidden, I = w->inter, Hq = w->heads, D = w->head_dim;
  const int B = st->batch, rows = B * T;
  if (fmt == FMT_W4A16 && w->fp8_act != 0) fmt = FMT_W4A8;  // mxfp4_direct (checked by llm_format) is not consulted
  if (fmt == FMT_W8A8 || fmt == FMT_W4A8)
    SRGPT_CHECK(Hd % 128 == 0 && I % 128 == 0 && (Hq * D) % 128 == 0 && Hd >= 256 && I >= 256 && Hq * D >= 256,
                SRGPT_ERR_UNSUPPORTED, "srgpt_llm_prefill: fp8_act needs hidden, inter and heads * head_dim to be multiples of 128");
  const bool wide = Hd > 16384 || I > 16384;  // the fused quantisation kernels hold rows of up to 16384 columns
  const size_t es = dtype_size(dt);
  hipStream_t s = as_stream(stream);
  const LlmWs l = carve_llm(w, B, st->ws_tokens, st->ws);
  const Prefill p{w, st, l, fmt, B, T, rows, Hd, I, Hq * D, (Hq + 2 * w->kv_heads) * D, dt, stream,
                  append ? l.app_pos0 : nullptr, append ? l.app_kvlen : nullptr, append ? h_pos_max + T : T};
  const size_t hid_bytes = (size_t)rows * Hd * es;
  if (append) {
    SRGPT_CHECK(Hd % (16 / (int)es) == 0, SRGPT_ERR_ARG, "srgpt_llm_prefill_append: hidden %d not a multiple of 16 bytes", Hd);
    hipLaunchKernelGGL(append_begin_kernel, dim3(cdiv(B, 64)), dim3(64), 0, s, st->pos, lens, B, T, h_pos_max, st->max_pos, l.app_pos0,
                       l.app_kvlen, l.err);
    SRGPT_LAUNCH_CHECK();
    // the rows in the residual-stream buffer of the decode step are not st->tok's any more: a captured step re-embeds.  The error
    // word stays (sticky), and so do the decode tickets: every launch leaves them zero, re-arming here could hide an earlier failure
    SRGPT_HIP_TRY(hipMemsetAsync(l.tok_emb, 0xFF, (size_t)B * sizeof(int64_t), s), "srgpt_llm_prefill_append: resetting the embedded-token record");
  } else {  // the decode attention's arrival tickets / sync words must be zero before the first step: every prefill re-arms them, so a
     // caller-allocated (never zeroed) workspace or an aborted launch cannot leave the decode steps merging nothing
    size_t sync_bytes = 0;
    void* sync = srgpt_decode_attn_sync_words(l.dws, B, Hq, D, &sync_bytes);
    SRGPT_HIP_TRY(hipMemsetAsync(sync, 0, sync_bytes, s), "srgpt_llm_prefill: re-arming the decode tickets");
    // no embedding row is in place for the new sequences (-1 matches no token id)
    SRGPT_HIP_TRY(hipMemsetAsync(l.tok_emb, 0xFF, (size_t)B * sizeof(int64_t), s), "srgpt_llm_prefill: resetting the embedded-token record");
    SRGPT_HIP_TRY(hipMemsetAsync(l.err, 0, sizeof(int), s), "srgpt_llm_prefill: clearing the decode error word");
  }
  if (hipMemcpyAsync(l.x, inputs_embeds, hid_bytes, hipMemcpyDeviceToDevice, s) != hipSuccess) {
    srgpt_set_error("srgpt_llm_prefill: memcpy failed");
    return SRGPT_ERR_LAUNCH;
  }
  if (hidden_out) SRGPT_HIP_TRY(hipMemcpyAsync(hidden_out, l.x, hid_bytes, hipMemcpyDeviceToDevice, s), "srgpt_llm_prefill: hidden-state copy");
  for (int i = 0; i < w->layers; ++i) {
    switch (fmt) {
      case FMT_DTYPE: SRGPT_TRY(p.layer_dtype(i)); break;
      case FMT_W8A16: SRGPT_TRY(p.layer_w8a16(i)); break;
      case FMT_W8A8:
      case FMT_W4A8: SRGPT_TRY(wide ? p.layer_w8a8_wide(i) : p.layer_w8a8(i)); break;
      case FMT_W4A16: SRGPT_TRY(p.layer_w4a16(i)); break;
    }
    if (hidden_out)
      SRGPT_HIP_TRY(hipMemcpyAsync(reinterpret_cast<char*>(hidden_out) + (size_t)(i + 1) * hid_bytes, l.x, hid_bytes,
                                   hipMemcpyDeviceToDevice, s),
                    "srgpt_llm_prefill: hidden-state copy");
  }
  if (all_logits) {  // no split-K workspace in any format
    SRGPT_TRY(p.norm(w->final_norm));
    if (fmt == FMT_DTYPE)
      SRGPT_TRY(srgpt_gemm(l.h, w->lm_head, nullptr, nullptr, all_logits, rows, w->vocab, Hd, Hd, w->vocab, SRGPT_ACT_NONE, 0, 0, 1,
                           SRGPT_OUT_PLAIN, 0, nullptr, 0, dt, stream));
    else
      SRGPT_TRY(srgpt_gemm_w8(l.h, w->lm_head8, w->lm_head_scale, nullptr, nullptr, all_logits, rows, w->vocab, Hd, Hd, w->vocab,
                              SRGPT_ACT_NONE, 1, nullptr, 0, stream));
  }
  // last position of every sequence -> logits (final norm fused into the GEMV prologue)
  if (append) {  // row lens[b] - 1 of the segment; pos[b] += lens[b] (both as validated by the first launch)
    hipLaunchKernelGGL(append_end_kernel, dim3(B), dim3(256), 0, s, reinterpret_cast<const unsigned char*>(l.x), l.app_pos0, l.app_kvlen,
                       reinterpret_cast<unsigned char*>(l.last), st->pos, T, (int)((size_t)Hd * es));
    SRGPT_LAUNCH_CHECK();
  } else if (lens) {  // right-padded ragged batch: row b ends at lens[b] - 1 and decoding continues from position lens[b]
    SRGPT_CHECK(Hd % (16 / (int)es) == 0, SRGPT_ERR_ARG, "srgpt_llm_prefill_ragged: hidden %d not a multiple of 16 bytes", Hd);
    if (dt == SRGPT_BF16)
      hipLaunchKernelGGL(gather_last_rows_kernel<bf16_t>, dim3(B), dim3(256), 0, s, (const bf16_t*)l.x, lens, (bf16_t*)l.last,
                         st->pos, T, Hd);
    else
      hipLaunchKernelGGL(gather_last_rows_kernel<float>, dim3(B), dim3(256), 0, s, (const float*)l.x, lens, (float*)l.last,
                         st->pos, T, Hd);
    SRGPT_LAUNCH_CHECK();
  } else {
    if (hipMemcpy2DAsync(l.last, (size_t)Hd * es, reinterpret_cast<char*>(l.x) + (size_t)(T - 1) * Hd * es,
                         (size_t)T * Hd * es, (size_t)Hd * es, B, hipMemcpyDeviceToDevice, s) != hipSuccess) {
      srgpt_set_error("srgpt_llm_prefill: gather of last rows failed");
      return SRGPT_ERR_LAUNCH;
    }
    hipLaunchKernelGGL(set_int_kernel, dim3(cdiv(B, 64)), dim3(64), 0, s, st->pos, B, T);
    SRGPT_LAUNCH_CHECK();
  }
  if (fmt == FMT_DTYPE)
    return srgpt_gemv(l.last, w->lm_head, w->final_norm, w->rms_eps, nullptr, st->logits, B, w->vocab, Hd, 0, 1, dt, stream);
  return srgpt_gemv_w8(l.last, w->lm_head8, w->lm_head_scale, w->final_norm, w->rms_eps, nullptr, st->logits, B, w->vocab, Hd, 0, 1,
                       stream);
}

extern "C" int srgpt_llm_prefill(const srgpt_llm_weights* w, srgpt_llm_state* st, const void* inputs_embeds, int T,
                                 float* all_logits, void* hidden_out, srgpt_stream_t stream) {
  return prefill_impl(w, st, inputs_embeds, T, nullptr, -1, all_logits, hidden_out, stream);
}

extern "C" int srgpt_llm_prefill_ragged(const srgpt_llm_weights* w, srgpt_llm_state* st, const void* inputs_embeds, int T,
                                        const int* lens, float* all_logits, void* hidden_out, srgpt_stream_t stream) {
  SRGPT_CHECK(lens, SRGPT_ERR_ARG, "srgpt_llm_prefill_ragged: lens is null");
  return prefill_impl(w, st, inputs_embeds, T, lens, -1, all_logits, hidden_out, stream);
}

extern "C" int srgpt_llm_prefill_append(const srgpt_llm_weights* w, srgpt_llm_state* st, const void* inputs_embeds, int T, const int* lens,
                                        int h_pos_max, float* all_logits, void* hidden_out, srgpt_stream_t stream) {
  SRGPT_CHECK(h_pos_max >= 0, SRGPT_ERR_ARG, "srgpt_llm_prefill_append: h_pos_max=%d is negative", h_pos_max);
  return prefill_impl(w, st, inputs_embeds, T, lens, h_pos_max, all_logits, hidden_out, stream);
}

// every pick entry point, on the host before any launch: a known sampler kind, a valid state, (full sampler, sampling on) a
// vocabulary it can hold, and (processors on) a history (st->out_ids, max_new ids per row) that fits their kernel
static int check_pick(const srgpt_llm_weights* w, const srgpt_llm_state* st, Pick p, const char* fn) {
  SRGPT_CHECK(p.sampler == SRGPT_SAMPLER_TOPK64 || p.sampler == SRGPT_SAMPLER_FULL, SRGPT_ERR_ARG, "%s: unknown sampler kind %d", fn,
              p.sampler);
  SRGPT_TRY(check_llm(w, st));
  if (st->sampling && p.sampler == SRGPT_SAMPLER_FULL) SRGPT_TRY(pick_check_vocab(w->vocab, fn));
  SRGPT_CHECK(!p.lp || (st->max_new > 0 && st->max_new <= srgpt_logits_proc_max_history()), SRGPT_ERR_UNSUPPORTED,
              "%s: logits processors over max_new = %d ids (served: 1 .. %d)", fn, st->max_new, srgpt_logits_proc_max_history());
  return SRGPT_OK;
}

static int sample_first_impl(const srgpt_llm_weights* w, srgpt_llm_state* st, Pick p, srgpt_stream_t stream) {
  hipStream_t s = as_stream(stream);
  hipLaunchKernelGGL(set_int_kernel, dim3(1), dim3(64), 0, s, st->step, 1, 0);  // the processors of the first token see 0 ids
  const LlmWs d = carve_llm(w, st->batch, st->ws_tokens, st->ws);
  return greedy_pick(w, st, d, 0, p, s);
}

extern "C" int srgpt_llm_sample_first_ex(const srgpt_llm_weights* w, srgpt_llm_state* st, int sampler, srgpt_stream_t stream) {
  SRGPT_TRY(check_pick(w, st, Pick{sampler, nullptr}, "srgpt_llm_sample_first_ex"));
  return sample_first_impl(w, st, Pick{sampler, nullptr}, stream);
}

extern "C" int srgpt_llm_sample_first_proc(const srgpt_llm_weights* w, srgpt_llm_state* st, int sampler, const srgpt_logits_proc* lp,
                                           srgpt_stream_t stream) {
  SRGPT_TRY(check_pick(w, st, Pick{sampler, lp}, "srgpt_llm_sample_first_proc"));
  return sample_first_impl(w, st, Pick{sampler, lp}, stream);
}

extern "C" int srgpt_llm_sample_first(const srgpt_llm_weights* w, srgpt_llm_state* st, srgpt_stream_t stream) {
  SRGPT_TRY(check_pick(w, st, Pick{SRGPT_SAMPLER_TOPK64, nullptr}, "srgpt_llm_sample_first"));
  return sample_first_impl(w, st, Pick{SRGPT_SAMPLER_TOPK64, nullptr}, stream);
}

namespace {

// ---- decode step ----
// The row buffers a decode-shaped step runs in: `rows` rows of the residual stream, of q/k/v, of the attention's output and of the
// MLP's activation, and the two row-statistics tables.  The plain step's are the state workspace's (LlmWs, rows = batch), a lookup
// step's its own workspace's (LookupWs, rows = batch * T).
struct StepRows {
  void *xd, *qkvd, *attnd, *actd;
  float* ss_attn;  // statistics of the rows after the attention block's residual add
  float* ss_mlp;   // ... after the MLP block's
  int rows;
};
StepRows step_rows(void* xd, void* qkvd, void* attnd, void* actd, float* rowss, int rows) {
  return StepRows{xd, qkvd, attnd, actd, rowss, rowss + (size_t)rows * SRGPT_ROWSS_STRIDE, rows};
}

// One product of a step, by the entry the step's route (gemv_route.h) and the weights allow, and the one sequence of products every
// decode-shaped step is made of.  pub: 2+ bf16 rows (the MFMA kernel): o_proj / down_proj publish the sum of squares of the rows
// they write (ss_out), the RMSNorm of the next product reads 512 partial sums per row (ss_in) instead of re-reading every row in
// every block (skinny.hip): the per-op form is srgpt_gemv_rowss.
struct DecodeStep {
  const srgpt_llm_weights* w;
  LlmFormat fmt;
  StepRows r;
  bool fp8, pub;
  bool p13;  // the plain one-row step of a bf16 engine in its dtype format: a matrix with a bound 13-bit copy is streamed from it
  bool w4p;  // MXFP4 engine, gemv_w4_step_route's MFMA leg: the layer products multiply the bound packed copies (then pub is true)
  srgpt_stream_t stream;

  // fp8: the matrices that are not MXFP4 (under FMT_W4A16: lm_head) are fp8.  plain_step: srgpt_llm_decode_step and its forms (the
  // lookup steps read the raw matrices whatever is bound)
  static DecodeStep make(const srgpt_llm_weights* w, LlmFormat fmt, const StepRows& r, srgpt_stream_t stream, bool plain_step) {
    const bool fp8 = fmt != FMT_DTYPE;
    const bool rowss = gemv_rowss_supported(r.rows, w->dtype == SRGPT_BF16, fp8, srgpt_device_cus());
    // MXFP4: all or nothing -- the MFMA leg only where the step has the rows for it, the statistics hand-off exists (lm_head is fp8)
    // and EVERY layer matrix has a packed copy of its shape; looked up on the host, at eager launch and at graph capture
    const bool w4p = fmt == FMT_W4A16 && rowss && r.rows >= W4_MFMA_MIN_ROWS &&
                     gemv_w4_step_route(r.rows, mxfp4_all_bound(w)).family == GEMV_W4_MFMA;
    const bool pub = fmt == FMT_W4A16 ? w4p : rowss;
    const bool p13 = plain_step && fmt == FMT_DTYPE && w->dtype == SRGPT_BF16 && r.rows == 1;
    return DecodeStep{w, fmt, r, fp8, pub, p13, w4p, stream};
  }

  // has every MXFP4 layer matrix of `w` a bound packed copy (srgpt_mxfp4_bind) of exactly its shape?
  static bool mxfp4_all_bound(const srgpt_llm_weights* w) {
    const int Hd = w->hidden, I = w->inter, HqD = w->heads * w->head_dim, QW = (w->heads + 2 * w->kv_heads) * w->head_dim;
    Mxfp4Binding b;
    for (int i = 0; i < w->layers; ++i)
      if (!srgpt_mxfp4_lookup(w->wqkv4[i], QW, Hd, 0, &b) || !srgpt_mxfp4_lookup(w->wo4[i], Hd, HqD, 0, &b) ||
          !srgpt_mxfp4_lookup(w->wgu4[i], I, Hd, 1, &b) || !srgpt_mxfp4_lookup(w->wdown4[i], Hd, I, 0, &b))
        return false;
    return w->layers > 0;
  }

  // packable: q/k/v, gate/up, down_proj and lm_head; o_proj is not -- the attention launch prefetches its RAW matrix into L2
  int gemv(const Mat& m, const void* x, const void* norm, const void* res, void* out, int N, int K, int swiglu, int f32,
           const float* ss_in, float* ss_out, bool packable = true) const {
    const bool wide = w->decode_pass_rows == GEMV_WIDE_ROWS;  // srgpt_llm_weights::decode_pass_rows: the wide entries (gemv_wide_route)
    if (m.w4 && w4p) {  // MXFP4 layer matrix on the MFMA leg: its packed copy, with the statistics hand-off of the other formats
      Mxfp4Binding b;
      SRGPT_CHECK(srgpt_mxfp4_lookup(m.w4, N, K, swiglu, &b), SRGPT_ERR_STATE, "decode step: an MXFP4 matrix was unbound while the step was being launched");
      return (wide ? srgpt_gemv_w4p_wide : srgpt_gemv_w4p)(x, b.packed, norm, w->rms_eps, res, out, r.rows, N, K, swiglu, f32, ss_in, ss_out,
                                                           stream);
    }
    if (m.w4)  // MXFP4 layer matrix on the VALU kernel, which neither reads nor publishes row statistics (pub is false)
      return srgpt_gemv_w4(x, m.w4, m.scale4, norm, w->rms_eps, res, out, r.rows, N, K, swiglu, f32, stream);
    if (pub)  // the MFMA kernel reads the packed copy of the fp8 bytes where there is one
      return (wide ? srgpt_gemv_rowss_wide : srgpt_gemv_rowss)(x, m.w, m.pk ? m.pk : m.w8, m.scale, norm, w->rms_eps, res, out, r.rows, N, K,
                                                               swiglu, f32, ss_in, ss_out, m.pk ? m.pk_rows : 0, stream);
    if (fp8) return srgpt_gemv_w8(x, m.w8, m.scale, norm, w->rms_eps, res, out, r.rows, N, K, swiglu, f32, stream);
    if (p13 && packable) {  // consulted on the host, at eager launch and at graph capture; srgpt_gemv itself never looks (it is the raw reference)
      Pack13Binding b;
      if (gemv_p13_eligible(r.rows, K) && srgpt_pack13_lookup(m.w, swiglu ? 2 * N : N, K, &b))
        return srgpt_gemv_p13(x, b.packed, b.meta, m.w, norm, w->rms_eps, res, out, N, K, swiglu, f32, stream);
    }
    return srgpt_gemv(x, m.w, norm, w->rms_eps, res, out, r.rows, N, K, swiglu, f32, w->dtype, stream);
  }

  // r.xd holds the rows' embeddings: the w->layers layers over the KV cache of `st`, then lm_head -> logits [rows, vocab] fp32.
  // attention(i, m, kc, vc) launches layer i's attention from r.qkvd over that layer's cache into r.attnd (m: the layer's matrices,
  // for the launch that prefetches o_proj) -- the one launch the steps differ in.  Layer 0's q/k/v normalises the embedding rows
  // itself; every later norm reads the statistics the product before it published.
  template <typename Attn>
  int layers_lm_head(const srgpt_llm_state* st, float* logits, Attn&& attention) const {
    const int Hd = w->hidden, I = w->inter, HqD = w->heads * w->head_dim, QW = (w->heads + 2 * w->kv_heads) * w->head_dim;
    const size_t layer_kv = (size_t)st->batch * w->kv_heads * st->max_pos * w->head_dim * dtype_size(w->dtype);
    for (int i = 0; i < w->layers; ++i) {
      char* kc = reinterpret_cast<char*>(st->kcache) + (size_t)i * layer_kv;
      char* vc = reinterpret_cast<char*>(st->vcache) + (size_t)i * layer_kv;
      const LayerMats m = layer_mats(w, fmt, i);
      SRGPT_TRY(gemv(m.qkv, r.xd, w->attn_norm[i], nullptr, r.qkvd, QW, Hd, 0, 0, i > 0 ? r.ss_mlp : nullptr, nullptr));
      SRGPT_TRY(attention(i, m, kc, vc));
      SRGPT_TRY(gemv(m.o, r.attnd, nullptr, r.xd, r.xd, Hd, HqD, 0, 0, nullptr, r.ss_attn, false));
      SRGPT_TRY(gemv(m.gu, r.xd, w->mlp_norm[i], nullptr, r.actd, I, Hd, 1, 0, r.ss_attn, nullptr));
      SRGPT_TRY(gemv(m.down, r.actd, nullptr, r.xd, r.xd, Hd, I, 0, 0, nullptr, r.ss_mlp));
    }
    return gemv(lm_head_mat(w), r.xd, w->final_norm, nullptr, logits, w->vocab, Hd, 0, 1, w->layers > 0 ? r.ss_mlp : nullptr, nullptr);
  }
};

}  // namespace

// embed_first = false: the residual-stream buffer already holds the embeddings of st->tok (written by the advance_kernel of the
// step before: the graph-captured greedy loop); the public entry always embeds (st->tok may have been set by the caller)
static int decode_step_impl(const srgpt_llm_weights* w, srgpt_llm_state* st, srgpt_stream_t stream, bool embed_first, Pick p) {
  LlmFormat fmt;
  SRGPT_TRY(llm_format(w, "srgpt_llm_decode_step", &fmt));
  const int dt = w->dtype, Hd = w->hidden, Hq = w->heads, Hkv = w->kv_heads, D = w->head_dim, B = st->batch;
  hipStream_t s = as_stream(stream);
  const LlmWs d = carve_llm(w, B, st->ws_tokens, st->ws);  // same carve as prefill (sized by ws_tokens)
  if (embed_first) {
    SRGPT_TRY(srgpt_embed_rows(w->embed, st->tok, d.xd, B, Hd, dt, stream));
    hipLaunchKernelGGL(record_embedded_kernel, dim3(cdiv(B, 64)), dim3(64), 0, s, st->tok, d.tok_emb, B);
    SRGPT_LAUNCH_CHECK();
  } else {  // captured step: one tiny launch that copies nothing unless the caller changed st->tok behind the graph's back
    hipLaunchKernelGGL(embed_sync_kernel, dim3(B < 64 ? B : 64), dim3(256), 0, s, st->tok, d.tok_emb,
                       reinterpret_cast<const unsigned char*>(w->embed), reinterpret_cast<unsigned char*>(d.xd), B,
                       (int)((size_t)Hd * dtype_size(dt)), (int64_t)w->vocab, d.err);
    SRGPT_LAUNCH_CHECK();
  }
  const bool fp8 = fmt != FMT_DTYPE, w4 = fmt == FMT_W4A16;
  const DecodeStep ds = DecodeStep::make(w, fmt, step_rows(d.xd, d.qkvd, d.attnd, d.actd, d.rowss, B), stream, true);
  // the attention launch also pulls o_proj's weights into L2 (HBM is idle while it runs).  Round 3 built the next step -- o_proj
  // itself inside this launch, weights in registers, agent-scope hand-off -- bit-exact and 3 us per layer SLOWER
  // (profiles/r03_fused_attention_oproj.txt)
  SRGPT_TRY(ds.layers_lm_head(st, st->logits, [&](int, const LayerMats& m, void* kc, void* vc) {
    return srgpt_decode_attention_pf(d.qkvd, kc, vc, st->pos, w->rope_cos, w->rope_sin, d.attnd, d.dws, B, Hq, Hkv, D, st->max_pos, dt,
                                     w4 ? m.o.w4 : fp8 ? m.o.w8 : m.o.w, Hd, Hq * D, w4 ? SRGPT_PREFETCH_W4 : fp8 ? 1 : 0, stream);
  }));
  return greedy_pick(w, st, d, 1, p, s);
}

extern "C" int srgpt_llm_decode_step_ex(const srgpt_llm_weights* w, srgpt_llm_state* st, int sampler, srgpt_stream_t stream) {
  SRGPT_TRY(check_pick(w, st, Pick{sampler, nullptr}, "srgpt_llm_decode_step_ex"));
  return decode_step_impl(w, st, stream, true, Pick{sampler, nullptr});
}

extern "C" int srgpt_llm_decode_step_proc(const srgpt_llm_weights* w, srgpt_llm_state* st, int sampler, const srgpt_logits_proc* lp,
                                          srgpt_stream_t stream) {
  SRGPT_TRY(check_pick(w, st, Pick{sampler, lp}, "srgpt_llm_decode_step_proc"));
  return decode_step_impl(w, st, stream, true, Pick{sampler, lp});
}

extern "C" int srgpt_llm_decode_step(const srgpt_llm_weights* w, srgpt_llm_state* st, srgpt_stream_t stream) {
  SRGPT_TRY(check_pick(w, st, Pick{SRGPT_SAMPLER_TOPK64, nullptr}, "srgpt_llm_decode_step"));
  return decode_step_impl(w, st, stream, true, Pick{SRGPT_SAMPLER_TOPK64, nullptr});
}

// Reads back the `bytes` of arrival tickets at `sync` behind the work queued on `stream` and checks them: between steps every ticket
// of a decode attention (the split that draws the last ticket merges and re-arms it) must be zero again -- a non-zero ticket means a
// launch was aborted or merged nothing, and every later step would silently use stale attention output.  `what` names the step in
// that message, `fn` the entry point in a failed HIP call's.  word (optional): one more device int read into *word_host by the same
// wait (`stream` is synchronised ONCE: the read-backs are queued, then one wait).
static int check_tickets(const void* sync, size_t bytes, srgpt_stream_t stream, const char* fn, const char* what,
                         const int* word = nullptr, int* word_host = nullptr) {
  std::vector<int> host(bytes / sizeof(int));
  hipError_t e = hipMemcpyAsync(host.data(), sync, bytes, hipMemcpyDeviceToHost, as_stream(stream));
  if (e == hipSuccess && word) e = hipMemcpyAsync(word_host, word, sizeof(int), hipMemcpyDeviceToHost, as_stream(stream));
  SRGPT_CHECK(e == hipSuccess, SRGPT_ERR_LAUNCH, "%s: copy failed: %s", fn, hipGetErrorString(e));
  e = hipStreamSynchronize(as_stream(stream));
  SRGPT_CHECK(e == hipSuccess, SRGPT_ERR_LAUNCH, "%s: synchronize failed: %s", fn, hipGetErrorString(e));
  for (size_t i = 0; i < host.size(); ++i)
    SRGPT_CHECK(host[i] == 0, SRGPT_ERR_STATE, "%s: arrival ticket %zu of %zu is %d between steps (expected 0)", what, i, host.size(),
                host[i]);
  return SRGPT_OK;
}

// Health of the decode steps since the last prefill: (1) the arrival tickets of the decode attention; (2) the sticky error word of
// the captured step (a caller-written token id outside the embedding table), of the samplers and of srgpt_llm_prefill_append.
extern "C" int srgpt_llm_decode_sync_state(const srgpt_llm_weights* w, const srgpt_llm_state* st, srgpt_stream_t stream) {
  SRGPT_TRY(check_llm(w, st));
  const LlmWs d = carve_llm(w, st->batch, st->ws_tokens, st->ws);
  size_t bytes = 0;
  void* sync = srgpt_decode_attn_sync_words(d.dws, st->batch, w->heads, w->head_dim, &bytes);
  int err = 0;
  SRGPT_TRY(check_tickets(sync, bytes, stream, "srgpt_llm_decode_sync_state", "decode step", d.err, &err));
  SRGPT_CHECK((err & ERR_APPEND_ROW) == 0, SRGPT_ERR_STATE,
              "srgpt_llm_prefill_append: a row's st->pos lay outside 0 .. h_pos_max or its length outside 1 .. T; the row was appended "
              "at a clamped position");
  SRGPT_CHECK((err & 4) == 0, SRGPT_ERR_UNSUPPORTED,
              "decode step: sampling parameters the device sampler does not serve (top_k > 64, or top_p < 1 without top_k): the draws "
              "used another distribution");
  SRGPT_CHECK((err & 2) == 0, SRGPT_ERR_STATE,
              "decode step: more than 256 vocabulary entries tie at the top-k threshold of a sampling step (kept set truncated)");
  SRGPT_CHECK((err & 1) == 0, SRGPT_ERR_STATE,
              "decode step: a token id written into st->tok lies outside the embedding table [0, %d); the step ran on a stale row",
              w->vocab);
  return SRGPT_OK;
}

// ================================================================================================
// the lookup steps: the next token and T - 1 drafted ones of each of B sequences through ONE pass over the weights (prompt-lookup
// decoding; B * T <= 16 rows, the skinny kernel's pass).  srgpt_lookup is the B = 1 form, srgpt_lookup_batch the per-row one.
// ================================================================================================
namespace {

// srgpt_lookup::ws (B = 1) / srgpt_lookup_batch::ws: B * T rows of the decode step's buffers and of the two row-statistics tables, the
// multi-token attention's workspace for (B, T) (its tickets zero between launches), the rows' pick partials and the [B, T] draft,
// row-id and count scratch
struct LookupWs {
  void *xd, *qkvd, *attnd, *actd;
  float* rowss;
  float* dws;
  float* amax_v;
  int* amax_i;
  int64_t *draft, *row_ids;
  int* n_draft;
  size_t total;
};
LookupWs carve_lookup(const srgpt_llm_weights* w, int B, int T, void* ws) {
  const size_t es = dtype_size(w->dtype);
  const size_t qkvw = (size_t)(w->heads + 2 * w->kv_heads) * w->head_dim;
  const size_t rows = (size_t)B * T;
  Carver c(ws);
  LookupWs l;
  l.xd = c.take(rows * w->hidden * es);
  l.qkvd = c.take(rows * qkvw * es);
  l.attnd = c.take(rows * w->heads * w->head_dim * es);
  l.actd = c.take(rows * w->inter * es);
  l.rowss = reinterpret_cast<float*>(c.take(2 * rows * SRGPT_ROWSS_STRIDE * sizeof(float)));
  l.dws = reinterpret_cast<float*>(c.take((size_t)srgpt_decode_attn_multi_ws_floats(B, T, w->heads, w->head_dim) * 4));
  l.amax_v = reinterpret_cast<float*>(c.take(rows * PICK_SLICES * 4));
  l.amax_i = reinterpret_cast<int*>(c.take(rows * PICK_SLICES * 4));
  l.draft = reinterpret_cast<int64_t*>(c.take(rows * 8));
  l.row_ids = reinterpret_cast<int64_t*>(c.take(rows * 8));
  l.n_draft = reinterpret_cast<int*>(c.take(rows * sizeof(int)));  // one count per sequence; up to 16 rows are one 256-byte unit
  l.total = c.off;
  return l;
}

// One lookup step as lookup_step_impl runs it, built from srgpt_lookup (B = 1) or srgpt_lookup_batch (steps != NULL)
struct LookupReq {
  int B, T, max_ngram;
  void* ws;
  float* logits;
  int* stats;
  const int64_t* prompt_ids;
  // batched: the row stride of prompt_ids and, on the device, every row's id count and emission count
  int ld_prompt;
  const int* n_prompt_dev;
  int* steps;
  // single: the id count (a host int of the public struct)
  int n_prompt;
  // the sampler kind of a sampled step and its workspace (the _ex entries)
  int sampler;
  void* sample_ws;
};
LookupReq lookup_req(const srgpt_lookup* lk, int sampler = SRGPT_SAMPLER_TOPK64, void* sample_ws = nullptr) {
  return LookupReq{1, lk->T, lk->max_ngram, lk->ws, lk->logits, lk->stats, lk->prompt_ids, 0, nullptr, nullptr, lk->n_prompt, sampler, sample_ws};
}
LookupReq lookup_req(const srgpt_lookup_batch* lk, int B, int sampler = SRGPT_SAMPLER_TOPK64, void* sample_ws = nullptr) {
  return LookupReq{B, lk->T, lk->max_ngram, lk->ws, lk->logits, lk->stats, lk->prompt_ids, lk->ld_prompt, lk->n_prompt, lk->steps, 0,
                   sampler, sample_ws};
}

}  // namespace

extern "C" int64_t srgpt_llm_lookup_ws_bytes(const srgpt_llm_weights* w, int T) {
  if (!w || T < 2 || T > srgpt_lookup_rows_max()) return -1;
  return (int64_t)carve_lookup(w, 1, T, nullptr).total;
}

extern "C" int64_t srgpt_llm_lookup_batch_ws_bytes(const srgpt_llm_weights* w, int B, int T) {
  if (!w || B < 1 || T < 2 || (int64_t)B * T > srgpt_lookup_rows_max()) return -1;
  return (int64_t)carve_lookup(w, B, T, nullptr).total;
}

// The parts the two host checks below share.  The checks themselves stay apart: they refuse overlapping things in different orders,
// and which refusal an argument set gets first is pinned.
// -- the multi-token attention serves T rows per sequence, and the pick a vocabulary of this size
static int check_lookup_rows(const srgpt_llm_weights* w, const srgpt_llm_state* st, int T, const char* fn) {
  const AttnDecodeMultiRoute r =
      attn_decode_multi_route(w->dtype == SRGPT_BF16, st->batch, T, w->heads, w->kv_heads, w->head_dim, st->max_pos);
  SRGPT_CHECK(r.status == ATTN_OK, SRGPT_ERR_UNSUPPORTED, "%s: T=%d rows x %d heads per kv head exceed the %d columns of the attention kernel",
              fn, T, r.G, ATTN_DEC_MULTI_COLS);
  return pick_check_vocab(w->vocab, fn);
}
static int check_max_ngram(int max_ngram, const char* fn) {
  SRGPT_CHECK(max_ngram >= 1 && max_ngram <= srgpt_lookup_ngram_max(), SRGPT_ERR_ARG, "%s: max_ngram=%d outside 1 .. %d", fn, max_ngram,
              srgpt_lookup_ngram_max());
  return SRGPT_OK;
}

// every single-sequence lookup entry point, on the host before any launch
static int check_lookup(const srgpt_llm_weights* w, const srgpt_llm_state* st, const srgpt_lookup* lk, const char* fn,
                        bool greedy_only = true) {
  SRGPT_CHECK(lk, SRGPT_ERR_ARG, "%s: null lookup block", fn);
  SRGPT_TRY(check_llm(w, st));
  SRGPT_CHECK(st->batch == 1, SRGPT_ERR_ARG, "%s: batch %d (the lookup step takes one sequence)", fn, st->batch);
  SRGPT_CHECK(lk->T >= 2, SRGPT_ERR_ARG, "%s: T=%d rows (the next token and at least one draft)", fn, lk->T);
  SRGPT_CHECK(lk->ws && lk->logits && lk->stats && (lk->prompt_ids || lk->n_prompt == 0) && lk->n_prompt >= 0, SRGPT_ERR_ARG,
              "%s: lookup block has null buffers", fn);
  SRGPT_TRY(check_max_ngram(lk->max_ngram, fn));
  SRGPT_CHECK(!greedy_only || !st->sampling, SRGPT_ERR_UNSUPPORTED,
              "%s: greedy only (st->sampling is set: the sampled step is srgpt_llm_lookup_step_ex)", fn);
  SRGPT_CHECK(lk->T <= srgpt_lookup_rows_max(), SRGPT_ERR_UNSUPPORTED, "%s: T=%d rows exceed %d", fn, lk->T, srgpt_lookup_rows_max());
  SRGPT_TRY(check_lookup_rows(w, st, lk->T, fn));
  LlmFormat fmt;
  return llm_format(w, fn, &fmt);
}

// the _ex entry points' check: a known sampler kind first, then check_lookup without the greedy-only refusal, then (sampling on)
// somewhere for the sampler to work
static int check_lookup_ex(const srgpt_llm_weights* w, const srgpt_llm_state* st, const srgpt_lookup* lk, int sampler,
                           const void* sample_ws, const char* fn) {
  SRGPT_CHECK(sampler == SRGPT_SAMPLER_TOPK64 || sampler == SRGPT_SAMPLER_FULL, SRGPT_ERR_ARG, "%s: unknown sampler kind %d", fn, sampler);
  SRGPT_TRY(check_lookup(w, st, lk, fn, false));
  SRGPT_CHECK(!st->sampling || sample_ws, SRGPT_ERR_ARG, "%s: st->sampling is set and sample_ws is null", fn);
  return SRGPT_OK;
}

// every batched lookup entry point, on the host before any launch
static int check_lookup_batch(const srgpt_llm_weights* w, const srgpt_llm_state* st, const srgpt_lookup_batch* lk, const char* fn,
                              bool greedy_only = true) {
  SRGPT_CHECK(lk, SRGPT_ERR_ARG, "%s: null lookup block", fn);
  SRGPT_TRY(check_llm(w, st));
  SRGPT_CHECK(lk->T >= 2, SRGPT_ERR_ARG, "%s: T=%d rows per sequence (the next token and at least one draft)", fn, lk->T);
  SRGPT_CHECK(!greedy_only || !st->sampling, SRGPT_ERR_UNSUPPORTED,
              "%s: greedy only (st->sampling is set: a sampled batch has one Philox counter, rows that emit different numbers of ids "
              "would need one each)", fn);
  SRGPT_CHECK((int64_t)st->batch * lk->T <= srgpt_lookup_rows_max(), SRGPT_ERR_UNSUPPORTED,
              "%s: batch %d x T=%d = %lld rows exceed the %d rows of one weight pass", fn, st->batch, lk->T, (long long)st->batch * lk->T,
              srgpt_lookup_rows_max());
  SRGPT_TRY(check_lookup_rows(w, st, lk->T, fn));
  SRGPT_CHECK(lk->ws && lk->logits && lk->stats && lk->steps && lk->n_prompt && (lk->prompt_ids || lk->ld_prompt == 0), SRGPT_ERR_ARG,
              "%s: lookup block has null buffers", fn);
  SRGPT_CHECK(lk->ld_prompt >= 0, SRGPT_ERR_ARG, "%s: ld_prompt=%d is negative", fn, lk->ld_prompt);
  SRGPT_TRY(check_max_ngram(lk->max_ngram, fn));
  LlmFormat fmt;
  return llm_format(w, fn, &fmt);
}

// the batched _ex entry points' check, built like check_lookup_ex
static int check_lookup_batch_ex(const srgpt_llm_weights* w, const srgpt_llm_state* st, const srgpt_lookup_batch* lk, int sampler,
                                 const void* sample_ws, const char* fn) {
  SRGPT_CHECK(sampler == SRGPT_SAMPLER_TOPK64 || sampler == SRGPT_SAMPLER_FULL, SRGPT_ERR_ARG, "%s: unknown sampler kind %d", fn, sampler);
  SRGPT_TRY(check_lookup_batch(w, st, lk, fn, false));
  SRGPT_CHECK(!st->sampling || sample_ws, SRGPT_ERR_ARG, "%s: st->sampling is set and sample_ws is null", fn);
  return SRGPT_OK;
}

extern "C" int64_t srgpt_llm_lookup_batch_sample_ws_bytes(const srgpt_llm_weights* w, int B, int T, int sampler) {
  if (!w || B < 1 || T < 2 || (int64_t)B * T > srgpt_lookup_rows_max()) return -1;
  if (sampler == SRGPT_SAMPLER_TOPK64) return srgpt_sample_ws_bytes(B * T);
  if (sampler == SRGPT_SAMPLER_FULL) return srgpt_sample_full_ws_bytes(B * T, w->vocab);
  return -1;
}

extern "C" int64_t srgpt_llm_lookup_sample_ws_bytes(const srgpt_llm_weights* w, int T, int sampler) {
  if (!w || T < 2 || T > srgpt_lookup_rows_max()) return -1;
  if (sampler == SRGPT_SAMPLER_TOPK64) return srgpt_sample_ws_bytes(T);
  if (sampler == SRGPT_SAMPLER_FULL) return srgpt_sample_full_ws_bytes(T, w->vocab);
  return -1;
}

// draft -> embed the R = B * T ids -> the layers and lm_head of the plain step over R rows, with the multi-token attention for B
// sequences of T rows (no o_proj prefetch blocks: 2+ rows take the skinny kernel) -> the rows' picks -> accept.  The forms differ in
// the first and the last launch only.  Draft: the batched kernel reads every row's id count from the device, the single one takes
// the public struct's host int.  Accept: greedy (st->sampling == NULL) the rows' argmax partials, then the single or the batched
// accept; sampled the sampler q.sampler over the R rows -- in its rows-are-steps mode, or (batched) as B sequences x T steps over
// q.steps (q.sample_ws: its own workspace, srgpt_llm_lookup_sample_ws_bytes / _batch_sample_ws_bytes; error bits go to the state's
// sticky word) -- then the single or the batched accept that advances the Philox counter.  The top-k-64 sampler's drawn ids go to the
// lookup workspace's row_ids, dead since the rows were embedded.
static int lookup_step_impl(const srgpt_llm_weights* w, srgpt_llm_state* st, const LookupReq& q, srgpt_stream_t stream) {
  const bool batched = q.steps != nullptr;
  LlmFormat fmt;
  SRGPT_TRY(llm_format(w, batched ? "srgpt_llm_lookup_step_batch" : "srgpt_llm_lookup_step", &fmt));
  const int dt = w->dtype, Hd = w->hidden, B = q.B, T = q.T, R = B * T;
  hipStream_t s = as_stream(stream);
  const LlmWs d = carve_llm(w, B, st->ws_tokens, st->ws);  // the state's sticky error word and embedded-token record
  const LookupWs l = carve_lookup(w, B, T, q.ws);
  if (batched)
    SRGPT_TRY(srgpt_lookup_draft_batch_launch(q.prompt_ids, q.ld_prompt, q.n_prompt_dev, st->out_ids, q.steps, B, st->max_new, T - 1,
                                              q.max_ngram, (int64_t)w->vocab, l.draft, l.n_draft, st->tok, l.row_ids, d.err, s));
  else
    SRGPT_TRY(srgpt_lookup_draft_launch(q.prompt_ids, q.n_prompt, st->out_ids, st->step, st->max_new, T - 1, q.max_ngram,
                                        (int64_t)w->vocab, l.draft, l.n_draft, st->tok, l.row_ids, d.err, s));
  SRGPT_TRY(srgpt_embed_rows(w->embed, l.row_ids, l.xd, R, Hd, dt, stream));
  const DecodeStep ds = DecodeStep::make(w, fmt, step_rows(l.xd, l.qkvd, l.attnd, l.actd, l.rowss, R), stream, false);
  SRGPT_TRY(ds.layers_lm_head(st, q.logits, [&](int, const LayerMats&, void* kc, void* vc) {
    return srgpt_decode_attention_multi(l.qkvd, kc, vc, st->pos, w->rope_cos, w->rope_sin, l.attnd, l.dws, B, T, w->heads, w->kv_heads,
                                        w->head_dim, st->max_pos, dt, stream);
  }));
  if (st->sampling) {
    const bool full = q.sampler == SRGPT_SAMPLER_FULL;
    float* pv;
    int* pi;
    if (full) {
      const SampleFullWs c = carve_sample_full_ws(q.sample_ws, R, w->vocab);
      pv = c.pv, pi = c.pi;
      SRGPT_TRY(batched ? srgpt_sample_full_seq_rows_launch(q.logits, st->sampling, q.steps, q.sample_ws, pv, pi, nullptr, B, T, w->vocab, s)
                        : srgpt_sample_full_rows_launch(q.logits, st->sampling, q.sample_ws, pv, pi, nullptr, T, w->vocab, s));
    } else {
      const SampleWs c = carve_sample_ws(q.sample_ws, R);
      pv = c.pv, pi = c.pi;
      SRGPT_TRY(batched ? srgpt_sample_seq_rows_launch(q.logits, st->sampling, q.steps, l.row_ids, q.sample_ws, pv, pi, d.err, B, T, w->vocab, s)
                        : srgpt_sample_rows_launch(q.logits, st->sampling, l.row_ids, q.sample_ws, pv, pi, d.err, T, w->vocab, s));
    }
    if (batched)
      return srgpt_lookup_accept_batch_sampled_launch(st->sampling, !full, l.row_ids, pv, pi, l.draft, l.n_draft, B, T, st->tok, st->out_ids,
                                                      st->pos, q.steps, st->step, st->max_new, st->max_pos, d.tok_emb, q.stats, s);
    return srgpt_lookup_accept_sampled_launch(st->sampling, !full, l.row_ids, pv, pi, l.draft, l.n_draft, T, st->tok, st->out_ids, st->pos,
                                              st->step, st->max_new, st->max_pos, d.tok_emb, q.stats, s);
  }
  hipLaunchKernelGGL(argmax_partial_kernel, dim3(PICK_SLICES, R), dim3(256), 0, s, q.logits, l.amax_v, l.amax_i, w->vocab);
  SRGPT_LAUNCH_CHECK();
  if (batched)
    return srgpt_lookup_accept_batch_launch(nullptr, l.amax_v, l.amax_i, l.draft, l.n_draft, B, T, st->tok, st->out_ids, st->pos, q.steps,
                                            st->step, st->max_new, st->max_pos, d.tok_emb, q.stats, s);
  return srgpt_lookup_accept_launch(nullptr, l.amax_v, l.amax_i, l.draft, l.n_draft, T, st->tok, st->out_ids, st->pos, st->step,
                                    st->max_new, st->max_pos, d.tok_emb, q.stats, s);
}

extern "C" int srgpt_llm_lookup_step(const srgpt_llm_weights* w, srgpt_llm_state* st, const srgpt_lookup* lk, srgpt_stream_t stream) {
  SRGPT_TRY(check_lookup(w, st, lk, "srgpt_llm_lookup_step"));
  return lookup_step_impl(w, st, lookup_req(lk), stream);
}

extern "C" int srgpt_llm_lookup_step_ex(const srgpt_llm_weights* w, srgpt_llm_state* st, const srgpt_lookup* lk, int sampler,
                                        void* sample_ws, srgpt_stream_t stream) {
  SRGPT_TRY(check_lookup_ex(w, st, lk, sampler, sample_ws, "srgpt_llm_lookup_step_ex"));
  return lookup_step_impl(w, st, lookup_req(lk, sampler, sample_ws), stream);
}

extern "C" int srgpt_llm_lookup_step_batch(const srgpt_llm_weights* w, srgpt_llm_state* st, const srgpt_lookup_batch* lk,
                                           srgpt_stream_t stream) {
  SRGPT_TRY(check_lookup_batch(w, st, lk, "srgpt_llm_lookup_step_batch"));
  return lookup_step_impl(w, st, lookup_req(lk, st->batch), stream);
}

extern "C" int srgpt_llm_lookup_step_batch_ex(const srgpt_llm_weights* w, srgpt_llm_state* st, const srgpt_lookup_batch* lk, int sampler,
                                              void* sample_ws, srgpt_stream_t stream) {
  SRGPT_TRY(check_lookup_batch_ex(w, st, lk, sampler, sample_ws, "srgpt_llm_lookup_step_batch_ex"));
  return lookup_step_impl(w, st, lookup_req(lk, st->batch, sampler, sample_ws), stream);
}

// srgpt_llm_decode_sync_state for a state a lookup step ran on: the (B, T) lookup workspace's own arrival tickets first, then
// everything the plain check reads (the state's tickets, its sticky error word)
static int lookup_sync_impl(const srgpt_llm_weights* w, const srgpt_llm_state* st, int B, int T, void* ws, srgpt_stream_t stream,
                            const char* fn, const char* what) {
  const LookupWs l = carve_lookup(w, B, T, ws);
  size_t bytes = 0;
  void* sync = srgpt_decode_attn_multi_sync_words(l.dws, B, T, w->heads, w->head_dim, &bytes);
  SRGPT_TRY(check_tickets(sync, bytes, stream, fn, what));
  return srgpt_llm_decode_sync_state(w, st, stream);
}

extern "C" int srgpt_llm_lookup_sync_state(const srgpt_llm_weights* w, const srgpt_llm_state* st, const srgpt_lookup* lk,
                                           srgpt_stream_t stream) {
  SRGPT_CHECK(lk && lk->ws && lk->T >= 2 && lk->T <= srgpt_lookup_rows_max(), SRGPT_ERR_ARG, "srgpt_llm_lookup_sync_state: bad lookup block");
  SRGPT_TRY(check_llm(w, st));
  return lookup_sync_impl(w, st, 1, lk->T, lk->ws, stream, "srgpt_llm_lookup_sync_state", "lookup step");
}

extern "C" int srgpt_llm_lookup_sync_state_batch(const srgpt_llm_weights* w, const srgpt_llm_state* st, const srgpt_lookup_batch* lk,
                                                 srgpt_stream_t stream) {
  SRGPT_CHECK(lk && lk->ws && lk->T >= 2, SRGPT_ERR_ARG, "srgpt_llm_lookup_sync_state_batch: bad lookup block");
  SRGPT_TRY(check_llm(w, st));
  SRGPT_CHECK((int64_t)st->batch * lk->T <= srgpt_lookup_rows_max(), SRGPT_ERR_ARG, "srgpt_llm_lookup_sync_state_batch: bad lookup block");
  return lookup_sync_impl(w, st, st->batch, lk->T, lk->ws, stream, "srgpt_llm_lookup_sync_state_batch", "batched lookup step");
}

// ================================================================================================
// hipGraph of one decode step
// ================================================================================================
// the graph entry points' check: somewhere to put the graph, then check_pick
static int check_graph(const srgpt_llm_weights* w, const srgpt_llm_state* st, Pick p, srgpt_graph** out, const char* fn) {
  SRGPT_CHECK(out, SRGPT_ERR_ARG, "srgpt_llm_decode_graph_create: null out");
  return check_pick(w, st, p, fn);
}

// the launches of `step()` on `stream`, captured and instantiated
template <typename F>
static int capture_graph(srgpt_stream_t stream, srgpt_graph** out, F&& step) {
  hipStream_t s = as_stream(stream);
  (void)srgpt_device_cus();  // make sure no device query happens inside the capture
  hipGraph_t graph = nullptr;
  if (hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal) != hipSuccess) {
    srgpt_set_error("hipStreamBeginCapture failed");
    return SRGPT_ERR_STATE;
  }
  const int rc = step();
  const hipError_t ee = hipStreamEndCapture(s, &graph);
  if (rc != SRGPT_OK) {
    if (graph) (void)hipGraphDestroy(graph);
    return rc;
  }
  if (ee != hipSuccess || !graph) {
    srgpt_set_error("hipStreamEndCapture failed: %s", hipGetErrorString(ee));
    return SRGPT_ERR_STATE;
  }
  hipGraphExec_t exec = nullptr;
  const hipError_t ei = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
  if (ei != hipSuccess) {
    (void)hipGraphDestroy(graph);
    srgpt_set_error("hipGraphInstantiate failed: %s", hipGetErrorString(ei));
    return SRGPT_ERR_STATE;
  }
  *out = new srgpt_graph{graph, exec};
  return SRGPT_OK;
}

static int graph_create_impl(const srgpt_llm_weights* w, srgpt_llm_state* st, Pick p, srgpt_stream_t stream, srgpt_graph** out) {
  LlmFormat fmt;  // incomplete fp8 weights never begin a capture (the step below resolves the format again)
  SRGPT_TRY(llm_format(w, "srgpt_llm_decode_step", &fmt));
  // replays continue from the token the previous step (or srgpt_llm_sample_first) picked: its embedding is already in place
  return capture_graph(stream, out, [&] { return decode_step_impl(w, st, stream, !advance_embeds(w, st), p); });
}

extern "C" int srgpt_llm_lookup_graph_create(const srgpt_llm_weights* w, srgpt_llm_state* st, const srgpt_lookup* lk,
                                             srgpt_stream_t stream, srgpt_graph** out) {
  SRGPT_CHECK(out, SRGPT_ERR_ARG, "srgpt_llm_lookup_graph_create: null out");
  SRGPT_TRY(check_lookup(w, st, lk, "srgpt_llm_lookup_graph_create"));
  return capture_graph(stream, out, [&] { return lookup_step_impl(w, st, lookup_req(lk), stream); });
}

extern "C" int srgpt_llm_lookup_graph_create_ex(const srgpt_llm_weights* w, srgpt_llm_state* st, const srgpt_lookup* lk, int sampler,
                                                void* sample_ws, srgpt_stream_t stream, srgpt_graph** out) {
  SRGPT_CHECK(out, SRGPT_ERR_ARG, "srgpt_llm_lookup_graph_create_ex: null out");
  SRGPT_TRY(check_lookup_ex(w, st, lk, sampler, sample_ws, "srgpt_llm_lookup_graph_create_ex"));
  return capture_graph(stream, out, [&] { return lookup_step_impl(w, st, lookup_req(lk, sampler, sample_ws), stream); });
}

extern "C" int srgpt_llm_lookup_graph_create_batch(const srgpt_llm_weights* w, srgpt_llm_state* st, const srgpt_lookup_batch* lk,
                                                   srgpt_stream_t stream, srgpt_graph** out) {
  SRGPT_CHECK(out, SRGPT_ERR_ARG, "srgpt_llm_lookup_graph_create_batch: null out");
  SRGPT_TRY(check_lookup_batch(w, st, lk, "srgpt_llm_lookup_graph_create_batch"));
  return capture_graph(stream, out, [&] { return lookup_step_impl(w, st, lookup_req(lk, st->batch), stream); });
}

extern "C" int srgpt_llm_lookup_graph_create_batch_ex(const srgpt_llm_weights* w, srgpt_llm_state* st, const srgpt_lookup_batch* lk,
                                                      int sampler, void* sample_ws, srgpt_stream_t stream, srgpt_graph** out) {
  SRGPT_CHECK(out, SRGPT_ERR_ARG, "srgpt_llm_lookup_graph_create_batch_ex: null out");
  SRGPT_TRY(check_lookup_batch_ex(w, st, lk, sampler, sample_ws, "srgpt_llm_lookup_graph_create_batch_ex"));
  return capture_graph(stream, out, [&] { return lookup_step_impl(w, st, lookup_req(lk, st->batch, sampler, sample_ws), stream); });
}

extern "C" int srgpt_llm_decode_graph_create_ex(const srgpt_llm_weights* w, srgpt_llm_state* st, int sampler, srgpt_stream_t stream,
                                                srgpt_graph** out) {
  SRGPT_TRY(check_graph(w, st, Pick{sampler, nullptr}, out, "srgpt_llm_decode_graph_create_ex"));
  return graph_create_impl(w, st, Pick{sampler, nullptr}, stream, out);
}

extern "C" int srgpt_llm_decode_graph_create_proc(const srgpt_llm_weights* w, srgpt_llm_state* st, int sampler,
                                                  const srgpt_logits_proc* lp, srgpt_stream_t stream, srgpt_graph** out) {
  SRGPT_TRY(check_graph(w, st, Pick{sampler, lp}, out, "srgpt_llm_decode_graph_create_proc"));
  return graph_create_impl(w, st, Pick{sampler, lp}, stream, out);
}

extern "C" int srgpt_llm_decode_graph_create(const srgpt_llm_weights* w, srgpt_llm_state* st, srgpt_stream_t stream,
                                             srgpt_graph** out) {
  SRGPT_TRY(check_graph(w, st, Pick{SRGPT_SAMPLER_TOPK64, nullptr}, out, "srgpt_llm_decode_graph_create"));
  return graph_create_impl(w, st, Pick{SRGPT_SAMPLER_TOPK64, nullptr}, stream, out);
}

extern "C" int srgpt_graph_launch(srgpt_graph* g, int times, srgpt_stream_t stream) {
  SRGPT_CHECK(g && times >= 0, SRGPT_ERR_ARG, "srgpt_graph_launch: bad args");
  for (int i = 0; i < times; ++i) {
    const hipError_t e = hipGraphLaunch(g->exec, as_stream(stream));
    if (e != hipSuccess) {
      srgpt_set_error("hipGraphLaunch failed: %s", hipGetErrorString(e));
      return SRGPT_ERR_LAUNCH;
    }
  }
  return SRGPT_OK;
}

extern "C" int srgpt_graph_destroy(srgpt_graph* g) {
  if (!g) return SRGPT_OK;
  (void)hipGraphExecDestroy(g->exec);  // best effort: nothing useful to report from a destructor path
  (void)hipGraphDestroy(g->graph);
  delete g;
  return SRGPT_OK;
}
