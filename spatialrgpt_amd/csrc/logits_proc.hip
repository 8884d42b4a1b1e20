// HF logits processors on the device (transformers 4.37.2 generation/logits_process.py), one launch in front of the pick of a decode
// step -- or on their own through srgpt_logits_process:
//   RepetitionPenaltyLogitsProcessor            score = gather(scores, ids); scatter(ids, score < 0 ? score * p : score / p)
//   NoRepeatNGramLogitsProcessor                every id that would complete a g-gram already in the history: -inf
//   MinLengthLogitsProcessor / MinNewTokens...  while fewer than min_new_tokens ids exist: every EOS id -inf
// One 256-thread block per sequence, three phases with a block barrier between them, so that the result does not depend on
// scheduling:
//   1  every history entry reads the ORIGINAL score of its id into LDS (HF's gather)
//   2  the penalised values are written (HF's scatter): two occurrences of an id write identical bits -- never a double penalty
//   3  the -inf writes (n-gram bans, EOS bans) go last: a ban wins over a penalty on the same entry
// The history is at most max_new ids: a few microseconds of work.  The parameter block lives in DEVICE memory (like srgpt_sampling),
// the history length may too (the decode step's counter): one captured graph serves every setting and every step.
#include "internal.h"

namespace {

constexpr int LP_THREADS = 256;
constexpr int LP_MAX_HIST = 12288;  // ids per row: their original scores fit 48 KiB of LDS
constexpr int LP_MAX_EOS = 8;       // srgpt_logits_proc::eos

__global__ __launch_bounds__(LP_THREADS) void logits_proc_kernel(float* __restrict__ scores, const srgpt_logits_proc* __restrict__ lp,
                                                                 const int64_t* __restrict__ ids, int ld, int n_host,
                                                                 const int* __restrict__ n_dev, int V) {
  extern __shared__ float orig[];  // [ld]: the score each history entry found
  float* row = scores + (size_t)blockIdx.x * V;
  const int64_t* h = ids + (size_t)blockIdx.x * ld;
  const int n = min(max(n_dev ? *n_dev : n_host, 0), ld);
  const float p = lp->repetition_penalty;
  const int g = lp->no_repeat_ngram;
  const bool penalise = p != 1.0f;

  if (penalise)
    for (int i = threadIdx.x; i < n; i += LP_THREADS) {
      const int64_t t = h[i];
      if (t >= 0 && t < V) orig[i] = row[t];
    }
  // every load above has returned before any wave stores (and below: every penalty store has landed before any ban is stored)
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (penalise)
    for (int i = threadIdx.x; i < n; i += LP_THREADS) {
      const int64_t t = h[i];
      if (t >= 0 && t < V) {
        const float s = orig[i];
        row[t] = s < 0.f ? s * p : s / p;  // a true fp32 division, as torch's
      }
    }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (g > 0 && n + 1 >= g) {
    // entry i starts a g-gram whose first g - 1 ids equal the last g - 1 of the history: its last id is banned
    const int64_t* tail = h + (n - (g - 1));
    for (int i = threadIdx.x; i + g - 1 < n; i += LP_THREADS) {
      bool same = true;
      for (int j = 0; j < g - 1 && same; ++j) same = h[i + j] == tail[j];
      const int64_t t = h[i + g - 1];
      if (same && t >= 0 && t < V) row[t] = -INFINITY;
    }
  }
  if (n < lp->min_new_tokens) {
    const int ne = min(max(lp->n_eos, 0), LP_MAX_EOS);
    for (int j = threadIdx.x; j < ne; j += LP_THREADS) {
      const int64_t t = lp->eos[j];
      if (t >= 0 && t < V) row[t] = -INFINITY;
    }
  }
}

}  // namespace

int srgpt_logits_proc_max_history() { return LP_MAX_HIST; }

// internal (model.hip): the launch on validated arguments; n_dev != NULL: the history length is read on the device
int srgpt_logits_proc_launch(float* scores, const srgpt_logits_proc* lp, const int64_t* ids, int ld, int n, const int* n_dev, int B, int V,
                             hipStream_t s) {
  SRGPT_CHECK(scores && lp && ids, SRGPT_ERR_ARG, "srgpt_logits_process: null pointer");
  SRGPT_CHECK(B > 0 && V > 0 && ld > 0, SRGPT_ERR_ARG, "srgpt_logits_process: empty shape (B %d, V %d, ld %d)", B, V, ld);
  SRGPT_CHECK(n >= 0 && n <= ld, SRGPT_ERR_ARG, "srgpt_logits_process: history length %d outside [0, %d]", n, ld);
  SRGPT_CHECK(ld <= LP_MAX_HIST, SRGPT_ERR_UNSUPPORTED, "srgpt_logits_process: a history of %d ids exceeds %d", ld, LP_MAX_HIST);
  hipLaunchKernelGGL(logits_proc_kernel, dim3(B), dim3(LP_THREADS), (size_t)ld * sizeof(float), s, scores, lp, ids, ld, n, n_dev, V);
  SRGPT_LAUNCH_CHECK();
  return SRGPT_OK;
}

extern "C" int srgpt_logits_process(float* scores, const srgpt_logits_proc* lp, const int64_t* ids, int ld, int n, const int* n_dev,
                                    int B, int V, srgpt_stream_t stream) {
  return srgpt_logits_proc_launch(scores, lp, ids, ld, n, n_dev, B, V, as_stream(stream));
}
