// Prompt-lookup decoding (HF generate(prompt_lookup_num_tokens = K), transformers 4.37 generation/candidate_generator.py
// PromptLookupCandidateGenerator): the two bookkeeping kernels around the T = K + 1 row decode step of model.hip.
//  1. lookup_draft_kernel  -- drafts up to K ids by matching the trailing n-gram of the sequence against the sequence itself;
//  2. lookup_accept_kernel -- compares the drafts with the model's picks, emits the agreed prefix + 1 and advances the state;
//     lookup_accept_sampled_kernel -- the same on picks that were DRAWN (a sampled request), and advances the Philox counter.
// One block each, nothing allocated, no host round trip: both sit inside the captured step.  The batched step's pair
// (lookup_draft_batch_kernel: one block per sequence, lookup_accept_batch_kernel: one thread per sequence) does the same for B
// sequences, lookup_accept_batch_sampled_kernel on draws (one Philox counter for all of them: draw_addr.h).  Each rule is written once: draft_sequence and accept_sequence; the kernels find their sequence's words and call them.
#include "common.h"
#include "internal.h"
#include "pick.h"

namespace {

constexpr int LOOKUP_NGRAM_MAX = 8;   // ids of the trailing window the matcher compares
constexpr int LOOKUP_ROWS_MAX = 16;   // T = K + 1 rows of a step: one wave of the accept block each

// The history is prompt_ids[n_prompt] followed by the first n_gen ids of out_ids.  An id outside [0, vocab) is a sentinel (-200, an
// id the embedding table does not hold): it never matches and is never drafted.
struct History {
  const int64_t* __restrict__ prompt;
  const int64_t* __restrict__ gen;
  int n_prompt, len;
  int64_t vocab;
  __device__ int64_t at(int i) const { return i < n_prompt ? prompt[i] : gen[i - n_prompt]; }
  __device__ bool real(int64_t id) const { return id >= 0 && id < vocab; }
};

// The draft of ONE sequence, by the whole block.  For n = min(max_ngram, len - 1) .. 1: the EARLIEST i with history[i .. i + n) == the
// last n ids (all real) and a real id behind it (i + n < len: the trailing n-gram itself never counts); the real ids that follow, at
// most K, are the drafts.  The position is a minimum over the matches: it does not depend on scheduling.  row_ids (optional, with
// tok) = the T = K + 1 ids the step embeds: *tok, the drafts, and behind them the last of these repeated (rows that can never be
// accepted).
__device__ void draft_sequence(const History& h, int K, int max_ngram, int64_t* __restrict__ draft, int* __restrict__ n_draft,
                               const int64_t* __restrict__ tok, int64_t* __restrict__ row_ids, int* __restrict__ err) {
  __shared__ int best;
  __shared__ int64_t tail[LOOKUP_NGRAM_MAX];
  int found = -1, found_n = 0;
  for (int n = min(max_ngram, h.len - 1); n >= 1 && found < 0; --n) {  // uniform over the block
    __syncthreads();
    if (threadIdx.x == 0) best = INT_MAX;
    if ((int)threadIdx.x < n) tail[threadIdx.x] = h.at(h.len - n + threadIdx.x);
    __syncthreads();
    bool tail_real = true;
    for (int j = 0; j < n; ++j) tail_real = tail_real && h.real(tail[j]);
    if (tail_real) {
      int mine = INT_MAX;
      for (int i = threadIdx.x; i + n < h.len && mine == INT_MAX; i += blockDim.x) {
        bool eq = h.real(h.at(i + n));
        for (int j = 0; j < n && eq; ++j) eq = h.at(i + j) == tail[j];
        if (eq) mine = i;  // ascending scan per thread: its earliest match
      }
      if (mine != INT_MAX) atomicMin(&best, mine);
    }
    __syncthreads();
    if (best != INT_MAX) {
      found = best;
      found_n = n;
    }
  }
  if (threadIdx.x != 0) return;
  int nd = 0;
  if (found >= 0)
    for (int i = found + found_n; nd < K && i < h.len && h.real(h.at(i)); ++i) draft[nd++] = h.at(i);
  for (int i = nd; i < K; ++i) draft[i] = -1;
  *n_draft = nd;
  if (row_ids) {
    int64_t t0 = *tok;
    if (!h.real(t0)) {  // a caller-written id outside the table cannot be embedded (the captured plain step's rule)
      if (err) atomicOr(err, 1);
      t0 = 0;
    }
    row_ids[0] = t0;
    for (int i = 0; i < K; ++i) row_ids[1 + i] = i < nd ? draft[i] : (nd > 0 ? draft[nd - 1] : t0);
  }
}

// one sequence: the history is prompt_ids[0 .. n_prompt) (a host count) and the first min(max(*step, 0), max_new) ids of out_ids
__global__ __launch_bounds__(1024) void lookup_draft_kernel(const int64_t* __restrict__ prompt_ids, int n_prompt,
                                                            const int64_t* __restrict__ out_ids, const int* __restrict__ step, int max_new,
                                                            int K, int max_ngram, int64_t vocab, int64_t* __restrict__ draft,
                                                            int* __restrict__ n_draft, const int64_t* __restrict__ tok,
                                                            int64_t* __restrict__ row_ids, int* __restrict__ err) {
  const int n_gen = min(max(*step, 0), max_new);
  draft_sequence(History{prompt_ids, out_ids, n_prompt, n_prompt + n_gen, vocab}, K, max_ngram, draft, n_draft, tok, row_ids, err);
}

// ---- the batched step: B sequences, T rows each (row r = b * T + t of every step buffer is token t of sequence b) ----
// sequence b = blockIdx.x over its own history: prompt_ids[b, 0 .. n_prompt[b]) (row stride ld_prompt; a device count outside
// 0 .. ld_prompt is clamped, so no id outside the row is read) followed by the first min(max(steps[b], 0), max_new) ids of
// out_ids[b, :].  draft [B, K], n_draft [B], row_ids [B, K + 1] (optional, with tok [B]).
__global__ __launch_bounds__(1024) void lookup_draft_batch_kernel(const int64_t* __restrict__ prompt_ids, int ld_prompt,
                                                                  const int* __restrict__ n_prompt, const int64_t* __restrict__ out_ids,
                                                                  const int* __restrict__ steps, int max_new, int K, int max_ngram,
                                                                  int64_t vocab, int64_t* __restrict__ draft, int* __restrict__ n_draft,
                                                                  const int64_t* __restrict__ tok, int64_t* __restrict__ row_ids,
                                                                  int* __restrict__ err) {
  const int b = blockIdx.x;
  const int np = min(max(n_prompt[b], 0), ld_prompt);
  const int n_gen = min(max(steps[b], 0), max_new);
  draft_sequence(History{prompt_ids + (size_t)b * ld_prompt, out_ids + (size_t)b * max_new, np, np + n_gen, vocab}, K, max_ngram,
                 draft + (size_t)b * K, n_draft + b, tok ? tok + b : nullptr, row_ids ? row_ids + (size_t)b * (K + 1) : nullptr, err);
}

// The accept blocks have one wave per row (rows <= LOOKUP_ROWS_MAX): picked[row] = ids[row] where the rows' picks are int64 ids
// already, or (ids == NULL) the merge of the row's PICK_SLICES partials in pv / pi (pick.h).  Ends in a barrier.
__device__ void gather_picks(const int64_t* __restrict__ ids, const float* __restrict__ pv, const int* __restrict__ pi, int rows,
                             int64_t* picked) {
  const int lane = threadIdx.x & 63, row = threadIdx.x >> 6;
  if (row < rows) {
    const int64_t t = ids ? ids[row] : (int64_t)pick_merge_row(pv + (size_t)row * PICK_SLICES, pi + (size_t)row * PICK_SLICES, PICK_SLICES, lane);
    if (lane == 0) picked[row] = t;
  }
  __syncthreads();
}

// The accept of ONE sequence, by one thread, over that sequence's own words (*step: the ids it has emitted, *pos, *tok, *tok_emb,
// out_ids: its row, draft: its T - 1 drafts, picked: its T rows' picks).  nd = the drafts that count: n_draft clamped to 0 .. T - 1
// and to the rows the cache had room for (P + i + 1 < max_pos: a row beyond the cache was not computed); n_acc = the longest prefix
// with draft[i] == picked[i], i < nd; the sequence emits picked[0 .. n_acc], cut at max_new.  A sequence whose count is outside
// 0 .. max_new - 1 is FROZEN (emitted = 0): nothing of it is written.  At max_new and beyond that is the run-ahead rule (the loop may
// launch once more than the request needs); a negative count is no state of a request, and nothing is written in front of its ids.
struct Accepted {
  int emitted, nd, n_acc;  // emitted == 0: frozen
};
__device__ Accepted accept_sequence(const int64_t* draft, int n_draft, const int64_t* picked, int T, int64_t* tok, int64_t* out_ids,
                                    int* pos, int* step, int max_new, int max_pos, int64_t* tok_emb) {
  const int s = *step;
  if (s < 0 || s >= max_new) return Accepted{0, 0, 0};
  const int P = *pos;
  const int nd = min(min(max(n_draft, 0), T - 1), max(max_pos - 1 - P, 0));
  int n_acc = 0;
  while (n_acc < nd && draft[n_acc] == picked[n_acc]) ++n_acc;
  const int emitted = min(n_acc + 1, max_new - s);
  for (int i = 0; i < emitted; ++i) out_ids[s + i] = picked[i];
  *step = s + emitted;
  *pos = P + emitted;
  *tok = picked[emitted - 1];
  if (tok_emb) *tok_emb = -1;  // the residual-stream buffer of the plain step holds no row of this token: a captured step re-embeds
  return Accepted{emitted, nd, n_acc};
}

__device__ void count_step(int* __restrict__ stats, int nd, int n_acc) {
  if (!stats) return;
  stats[0] += 1;
  stats[1] += nd;
  stats[2] += n_acc;
}

// picks (optional): the T rows' picks as srgpt_argmax leaves them; NULL: merged from the partials
__global__ __launch_bounds__(64 * LOOKUP_ROWS_MAX) void lookup_accept_kernel(const int64_t* __restrict__ picks, const float* __restrict__ pv,
                                                                             const int* __restrict__ pi, const int64_t* __restrict__ draft,
                                                                             const int* __restrict__ n_draft, int T, int64_t* __restrict__ tok,
                                                                             int64_t* __restrict__ out_ids, int* __restrict__ pos,
                                                                             int* __restrict__ step, int max_new, int max_pos,
                                                                             int64_t* __restrict__ tok_emb, int* __restrict__ stats) {
  __shared__ int64_t picked[LOOKUP_ROWS_MAX];
  gather_picks(picks, pv, pi, T, picked);
  if (threadIdx.x != 0) return;
  const Accepted a = accept_sequence(draft, *n_draft, picked, T, tok, out_ids, pos, step, max_new, max_pos, tok_emb);
  if (a.emitted) count_step(stats, a.nd, a.n_acc);
}

// the SAMPLED step: the T rows' picks are DRAWS, row t at Philox counter sp->counter + t (the samplers' rows-are-steps mode).  Where
// they lie is read from the parameter block, as advance_kernel (model.hip) does: the top-k-64 sampler (select_drew) with top_k >= 1
// left int64 ids in `drawn` (sample_select_kernel); its Gumbel mode and the full sampler left PICK_SLICES partials per row in pv / pi.
// Row t's draw is used only when rows 0 .. t - 1 agreed with their drafts: it is a draw from the model's distribution behind the
// emitted prefix (HF assisted decoding without candidate logits).  The counter advances by the ids emitted, so generated id i was
// drawn at c0 + i whatever the steps accepted, as in the plain sampled loop; the random numbers of a discarded row influenced nothing
// that was kept, and the next step's row 0 reads them again.
__global__ __launch_bounds__(64 * LOOKUP_ROWS_MAX) void lookup_accept_sampled_kernel(
    srgpt_sampling* __restrict__ sp, int select_drew, const int64_t* __restrict__ drawn, const float* __restrict__ pv,
    const int* __restrict__ pi, const int64_t* __restrict__ draft, const int* __restrict__ n_draft, int T, int64_t* __restrict__ tok,
    int64_t* __restrict__ out_ids, int* __restrict__ pos, int* __restrict__ step, int max_new, int max_pos, int64_t* __restrict__ tok_emb,
    int* __restrict__ stats) {
  __shared__ int64_t picked[LOOKUP_ROWS_MAX];
  gather_picks(select_drew && sp->top_k > 0 ? drawn : nullptr, pv, pi, T, picked);
  if (threadIdx.x != 0) return;
  const Accepted a = accept_sequence(draft, *n_draft, picked, T, tok, out_ids, pos, step, max_new, max_pos, tok_emb);
  if (!a.emitted) return;  // frozen: nothing is bumped, the counter included
  count_step(stats, a.nd, a.n_acc);
  sp->counter += (unsigned long long)a.emitted;
}

// Thread 0 of a batched accept, behind the sequences' accepts (s_steps: their counts now): *step = min over b of steps[b], the columns
// of out_ids every row has filled; stats += {1, the drafts, the accepted ones} of the rows that advanced, summed in row order.
__device__ void book_batch_step(const int* s_steps, const Accepted* s_acc, int B, int* __restrict__ step, int* __restrict__ stats) {
  int lo = INT_MAX, live = 0, nd = 0, n_acc = 0;
  for (int b = 0; b < B; ++b) {
    lo = min(lo, s_steps[b]);
    if (s_acc[b].emitted) {
      live = 1;
      nd += s_acc[b].nd;
      n_acc += s_acc[b].n_acc;
    }
  }
  *step = lo;
  if (live) count_step(stats, nd, n_acc);
}

// One wave per row gathers the B * T rows' picks (B * T <= LOOKUP_ROWS_MAX); then thread b accepts sequence b: its own steps[b], pos[b],
// tok[b], tok_emb[b], out_ids[b, :], its T - 1 drafts and picks b * T .. .  A frozen sequence is neither written nor counted (the
// run-ahead rule, per row -- a row that accepted more than the others gets there first and waits).  Then thread 0: book_batch_step.
__global__ __launch_bounds__(64 * LOOKUP_ROWS_MAX) void lookup_accept_batch_kernel(
    const int64_t* __restrict__ picks, const float* __restrict__ pv, const int* __restrict__ pi, const int64_t* __restrict__ draft,
    const int* __restrict__ n_draft, int B, int T, int64_t* __restrict__ tok, int64_t* __restrict__ out_ids, int* __restrict__ pos,
    int* __restrict__ steps, int* __restrict__ step, int max_new, int max_pos, int64_t* __restrict__ tok_emb, int* __restrict__ stats) {
  __shared__ int64_t picked[LOOKUP_ROWS_MAX];
  __shared__ int s_steps[LOOKUP_ROWS_MAX];
  __shared__ Accepted s_acc[LOOKUP_ROWS_MAX];  // per sequence
  gather_picks(picks, pv, pi, B * T, picked);
  if ((int)threadIdx.x < B) {
    const int b = threadIdx.x;
    s_acc[b] = accept_sequence(draft + (size_t)b * (T - 1), n_draft[b], picked + b * T, T, tok + b, out_ids + (size_t)b * max_new, pos + b,
                               steps + b, max_new, max_pos, tok_emb ? tok_emb + b : nullptr);
    s_steps[b] = steps[b];
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  book_batch_step(s_steps, s_acc, B, step, stats);
}

// the SAMPLED batched step: the B * T rows' picks are DRAWS, row (b, t) at draw_addr.h's address -- sp->counter names the draw of
// column m = min over b of max(steps[b], 0) of out_ids, and the row reads (counter + max(steps[b], 0) - m + t, b), the samplers'
// PICK_ROWS_SEQ_STEPS mode.  Where the picks lie is read from the parameter block as lookup_accept_sampled_kernel reads it.  The
// sequences' accepts and thread 0's book_batch_step are lookup_accept_batch_kernel's; then sp->counter += m after - m before, taken
// from the steps[] values on both sides of the accepts, so the counter goes on naming column m: generated id i of sequence b was
// drawn at (c0 + i, b) whatever the steps accepted, as in the plain sampled batched loop.  A frozen sequence is neither written nor
// counted; when every one is frozen m stays, so the advance is 0 and the counter stays.
__global__ __launch_bounds__(64 * LOOKUP_ROWS_MAX) void lookup_accept_batch_sampled_kernel(
    srgpt_sampling* __restrict__ sp, int select_drew, const int64_t* __restrict__ drawn, const float* __restrict__ pv,
    const int* __restrict__ pi, const int64_t* __restrict__ draft, const int* __restrict__ n_draft, int B, int T, int64_t* __restrict__ tok,
    int64_t* __restrict__ out_ids, int* __restrict__ pos, int* __restrict__ steps, int* __restrict__ step, int max_new, int max_pos,
    int64_t* __restrict__ tok_emb, int* __restrict__ stats) {
  __shared__ int64_t picked[LOOKUP_ROWS_MAX];
  __shared__ int s_before[LOOKUP_ROWS_MAX], s_steps[LOOKUP_ROWS_MAX];
  __shared__ Accepted s_acc[LOOKUP_ROWS_MAX];  // per sequence
  gather_picks(select_drew && sp->top_k > 0 ? drawn : nullptr, pv, pi, B * T, picked);
  if ((int)threadIdx.x < B) {
    const int b = threadIdx.x;
    s_before[b] = steps[b];
    s_acc[b] = accept_sequence(draft + (size_t)b * (T - 1), n_draft[b], picked + b * T, T, tok + b, out_ids + (size_t)b * max_new, pos + b,
                               steps + b, max_new, max_pos, tok_emb ? tok_emb + b : nullptr);
    s_steps[b] = steps[b];
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  book_batch_step(s_steps, s_acc, B, step, stats);
  sp->counter += draw_advance(draw_column(s_before, B), draw_column(s_steps, B));
}

int check_draft_args(int n_prompt, int max_new, int K, int max_ngram, int64_t vocab, const char* fn) {
  SRGPT_CHECK(n_prompt >= 0 && max_new > 0 && vocab > 0, SRGPT_ERR_ARG, "%s: bad sizes n_prompt=%d max_new=%d vocab=%lld", fn, n_prompt,
              max_new, (long long)vocab);
  SRGPT_CHECK(K >= 1 && K < LOOKUP_ROWS_MAX, SRGPT_ERR_ARG, "%s: K=%d drafts outside 1 .. %d", fn, K, LOOKUP_ROWS_MAX - 1);
  SRGPT_CHECK(max_ngram >= 1 && max_ngram <= LOOKUP_NGRAM_MAX, SRGPT_ERR_ARG, "%s: max_ngram=%d outside 1 .. %d", fn, max_ngram,
              LOOKUP_NGRAM_MAX);
  return SRGPT_OK;
}

}  // namespace

int srgpt_lookup_rows_max() { return LOOKUP_ROWS_MAX; }
int srgpt_lookup_ngram_max() { return LOOKUP_NGRAM_MAX; }

int srgpt_lookup_draft_launch(const int64_t* prompt_ids, int n_prompt, const int64_t* out_ids, const int* step, int max_new, int K,
                              int max_ngram, int64_t vocab, int64_t* draft, int* n_draft, const int64_t* tok, int64_t* row_ids, int* err,
                              hipStream_t s) {
  hipLaunchKernelGGL(lookup_draft_kernel, dim3(1), dim3(1024), 0, s, prompt_ids, n_prompt, out_ids, step, max_new, K, max_ngram, vocab,
                     draft, n_draft, tok, row_ids, err);
  SRGPT_LAUNCH_CHECK();
  return SRGPT_OK;
}

int srgpt_lookup_accept_launch(const int64_t* picks, const float* pv, const int* pi, const int64_t* draft, const int* n_draft, int T,
                               int64_t* tok, int64_t* out_ids, int* pos, int* step, int max_new, int max_pos, int64_t* tok_emb, int* stats,
                               hipStream_t s) {
  hipLaunchKernelGGL(lookup_accept_kernel, dim3(1), dim3(64 * LOOKUP_ROWS_MAX), 0, s, picks, pv, pi, draft, n_draft, T, tok, out_ids, pos,
                     step, max_new, max_pos, tok_emb, stats);
  SRGPT_LAUNCH_CHECK();
  return SRGPT_OK;
}

int srgpt_lookup_accept_sampled_launch(srgpt_sampling* sp, int select_drew, const int64_t* drawn, const float* pv, const int* pi,
                                       const int64_t* draft, const int* n_draft, int T, int64_t* tok, int64_t* out_ids, int* pos, int* step,
                                       int max_new, int max_pos, int64_t* tok_emb, int* stats, hipStream_t s) {
  hipLaunchKernelGGL(lookup_accept_sampled_kernel, dim3(1), dim3(64 * LOOKUP_ROWS_MAX), 0, s, sp, select_drew, drawn, pv, pi, draft,
                     n_draft, T, tok, out_ids, pos, step, max_new, max_pos, tok_emb, stats);
  SRGPT_LAUNCH_CHECK();
  return SRGPT_OK;
}

int srgpt_lookup_accept_batch_sampled_launch(srgpt_sampling* sp, int select_drew, const int64_t* drawn, const float* pv, const int* pi,
                                             const int64_t* draft, const int* n_draft, int B, int T, int64_t* tok, int64_t* out_ids,
                                             int* pos, int* steps, int* step, int max_new, int max_pos, int64_t* tok_emb, int* stats,
                                             hipStream_t s) {
  hipLaunchKernelGGL(lookup_accept_batch_sampled_kernel, dim3(1), dim3(64 * LOOKUP_ROWS_MAX), 0, s, sp, select_drew, drawn, pv, pi, draft,
                     n_draft, B, T, tok, out_ids, pos, steps, step, max_new, max_pos, tok_emb, stats);
  SRGPT_LAUNCH_CHECK();
  return SRGPT_OK;
}

int srgpt_lookup_draft_batch_launch(const int64_t* prompt_ids, int ld_prompt, const int* n_prompt, const int64_t* out_ids, const int* steps,
                                    int B, int max_new, int K, int max_ngram, int64_t vocab, int64_t* draft, int* n_draft,
                                    const int64_t* tok, int64_t* row_ids, int* err, hipStream_t s) {
  hipLaunchKernelGGL(lookup_draft_batch_kernel, dim3(B), dim3(1024), 0, s, prompt_ids, ld_prompt, n_prompt, out_ids, steps, max_new, K,
                     max_ngram, vocab, draft, n_draft, tok, row_ids, err);
  SRGPT_LAUNCH_CHECK();
  return SRGPT_OK;
}

int srgpt_lookup_accept_batch_launch(const int64_t* picks, const float* pv, const int* pi, const int64_t* draft, const int* n_draft, int B,
                                     int T, int64_t* tok, int64_t* out_ids, int* pos, int* steps, int* step, int max_new, int max_pos,
                                     int64_t* tok_emb, int* stats, hipStream_t s) {
  hipLaunchKernelGGL(lookup_accept_batch_kernel, dim3(1), dim3(64 * LOOKUP_ROWS_MAX), 0, s, picks, pv, pi, draft, n_draft, B, T, tok,
                     out_ids, pos, steps, step, max_new, max_pos, tok_emb, stats);
  SRGPT_LAUNCH_CHECK();
  return SRGPT_OK;
}

extern "C" int srgpt_lookup_draft(const int64_t* prompt_ids, int n_prompt, const int64_t* out_ids, const int* step, int max_new, int K,
                                  int max_ngram, int64_t vocab, int64_t* draft, int* n_draft, srgpt_stream_t stream) {
  SRGPT_CHECK((prompt_ids || n_prompt == 0) && out_ids && step && draft && n_draft, SRGPT_ERR_ARG, "srgpt_lookup_draft: null pointer");
  SRGPT_TRY(check_draft_args(n_prompt, max_new, K, max_ngram, vocab, "srgpt_lookup_draft"));
  return srgpt_lookup_draft_launch(prompt_ids, n_prompt, out_ids, step, max_new, K, max_ngram, vocab, draft, n_draft, nullptr, nullptr,
                                   nullptr, as_stream(stream));
}

extern "C" int srgpt_lookup_accept(const int64_t* picks, const int64_t* draft, const int* n_draft, int T, int64_t* tok, int64_t* out_ids,
                                   int* pos, int* step, int max_new, int max_pos, int64_t* tok_emb, int* stats, srgpt_stream_t stream) {
  SRGPT_CHECK(picks && draft && n_draft && tok && out_ids && pos && step, SRGPT_ERR_ARG, "srgpt_lookup_accept: null pointer");
  SRGPT_CHECK(T >= 2 && T <= LOOKUP_ROWS_MAX && max_new > 0 && max_pos > 0, SRGPT_ERR_ARG,
              "srgpt_lookup_accept: bad sizes T=%d (2 .. %d) max_new=%d max_pos=%d", T, LOOKUP_ROWS_MAX, max_new, max_pos);
  return srgpt_lookup_accept_launch(picks, nullptr, nullptr, draft, n_draft, T, tok, out_ids, pos, step, max_new, max_pos, tok_emb, stats,
                                    as_stream(stream));
}

extern "C" int srgpt_lookup_draft_batch(const int64_t* prompt_ids, int ld_prompt, const int* n_prompt, const int64_t* out_ids,
                                        const int* steps, int B, int max_new, int K, int max_ngram, int64_t vocab, int64_t* draft,
                                        int* n_draft, srgpt_stream_t stream) {
  SRGPT_CHECK((prompt_ids || ld_prompt == 0) && n_prompt && out_ids && steps && draft && n_draft, SRGPT_ERR_ARG,
              "srgpt_lookup_draft_batch: null pointer");
  SRGPT_CHECK(B >= 1 && B <= LOOKUP_ROWS_MAX && ld_prompt >= 0, SRGPT_ERR_ARG, "srgpt_lookup_draft_batch: bad sizes B=%d (1 .. %d) ld_prompt=%d",
              B, LOOKUP_ROWS_MAX, ld_prompt);
  SRGPT_TRY(check_draft_args(0, max_new, K, max_ngram, vocab, "srgpt_lookup_draft_batch"));
  return srgpt_lookup_draft_batch_launch(prompt_ids, ld_prompt, n_prompt, out_ids, steps, B, max_new, K, max_ngram, vocab, draft, n_draft,
                                         nullptr, nullptr, nullptr, as_stream(stream));
}

extern "C" int srgpt_lookup_accept_batch(const int64_t* picks, const int64_t* draft, const int* n_draft, int B, int T, int64_t* tok,
                                         int64_t* out_ids, int* pos, int* steps, int* step, int max_new, int max_pos, int64_t* tok_emb,
                                         int* stats, srgpt_stream_t stream) {
  SRGPT_CHECK(picks && draft && n_draft && tok && out_ids && pos && steps && step, SRGPT_ERR_ARG, "srgpt_lookup_accept_batch: null pointer");
  SRGPT_CHECK(B >= 1 && T >= 2 && max_new > 0 && max_pos > 0, SRGPT_ERR_ARG, "srgpt_lookup_accept_batch: bad sizes B=%d T=%d (2 ..) max_new=%d max_pos=%d",
              B, T, max_new, max_pos);
  SRGPT_CHECK((int64_t)B * T <= LOOKUP_ROWS_MAX, SRGPT_ERR_UNSUPPORTED, "srgpt_lookup_accept_batch: B=%d x T=%d rows exceed %d", B, T,
              LOOKUP_ROWS_MAX);
  return srgpt_lookup_accept_batch_launch(picks, nullptr, nullptr, draft, n_draft, B, T, tok, out_ids, pos, steps, step, max_new, max_pos,
                                          tok_emb, stats, as_stream(stream));
}
