// Device-side sampling of the next token: temperature -> top-k -> top-p -> categorical draw, the warper chain HF's
// GenerationMixin.sample applies for the reference's interactive callers (demo/gradio_web_server_multi.py:202-213: do_sample,
// temperature 0.2, top_k = the transformers==4.37.2 default 50; llava/eval/model_vqa.py:66-80: temperature / top_p / num_beams).
// Round 3 ran this as torch ops per token outside the captured step; here it is three launches INSIDE the hipGraph of the decode
// step, driven by a device-resident parameter block (one graph serves every temperature / top-k / top-p / seed).
//
//   launch 1  sample_partial_kernel   grid (128 vocabulary slices, batch): the slice's scores logits / T as order-preserving
//             integer keys in LDS, the slice's top-k by a 4-pass radix select (LDS histograms, one wave scans the 256 bins),
//             <= 64 candidates (key, index) per slice (ties at the slice's k-th score included while the slots last).  top_k = 0 (no filter, top_p off): the Gumbel-max trick -- argmax of
//             score + Gumbel noise IS a draw from softmax(score) -- as per-slice maxima for the greedy merge kernel.
//   launch 2  sample_select_kernel    one block per sequence: the 128 x 64 candidates in LDS, the global k-th largest score by the
//             same radix select, kept = every candidate >= it (ties kept, like TopKLogitsWarper's `scores < kth` mask), rank-sorted
//             by (score desc, index desc: torch.sort's order among ties, reversed) -- deterministic whatever order the LDS atomics
//             appended them in; then, on one thread over
//             <= 256 entries: top-p exactly as TopPLogitsWarper (ascending cumulative softmax, remove <= 1 - top_p, never the
//             largest), and the draw by inverse CDF on one Philox4x32-10 uniform.
//   launch 3  advance_kernel (model.hip) books the token like the greedy path and advances the Philox counter.
// What the launches share with the argmax -- slice count and bounds, the vocabulary limit, the (value, index) tie rule and its
// reductions, the Gumbel key, both workspace layouts -- is pick.h; sample_merge_kernel is launch 3 of the stand-alone ops.
// That sampler serves top_k 1 .. 64 (any top_p) and pure temperature sampling.  The FULL sampler below (srgpt_sample_full, the
// decode step's SRGPT_SAMPLER_FULL) serves every setting over the whole vocabulary:
//   launch 1  sample_full_threshold_kernel  one 1024-thread block per sequence: keys of logits / T to the workspace; the kept set as
//             ONE (key, index) threshold pair -- top-k by a 12 + 10 + 10-bit radix select of counts, top-p by the same digit walk
//             over 64-bit fixed-point softmax mass (integer sums: bit-stable replays), a tie group cut by top-p losing its lowest
//             indices first (CPU torch.sort's ascending order).
//   launch 2  sample_full_draw_kernel       grid (128 slices, batch): masked Gumbel-max, per-slice (value, index) for the greedy
//             merge (advance_kernel / sample_merge_kernel), Philox addressed like the top_k = 0 path.
// WHAT THE ROWS ARE (template argument MODE of the kernels that draw, PickRows of pick.h).  PICK_ROWS_SEQS: the sequences of one step.
// PICK_ROWS_STEPS (srgpt_sample_rows / srgpt_sample_full_rows and the sampled lookup step of model.hip): T successive steps of ONE
// sequence, row t reads the stream below at (step counter + t, sequence 0) -- what a one-row call at that counter reads.
// PICK_ROWS_SEQ_STEPS (srgpt_sample_seq_rows / srgpt_sample_full_seq_rows and the batched sampled lookup step): B sequences x T
// successive steps, row b * T + t at draw_addr.h's address over the sequences' emission counts, which these instantiations take as
// one more kernel argument (PickSeqs); they leave the counter alone.  Nothing else differs between the three, and the first two are
// the kernels as they were, instruction for instruction.
// Randomness: Philox4x32-10 keyed by the caller's seed, counter = (step counter, sequence, vocabulary index | ~0): reproducible for
// a given seed, independent across steps / sequences / slices; torch's generator cannot be matched (HF itself draws differently
// on CPU and GPU) -- parity is the KEPT SET (bit-equal to HF's warpers on the same logits), the drawn DISTRIBUTION (chi-square) and
// the TOKEN itself: tests/draw_ref.py restates the address, the inverse-CDF walk and the Gumbel key on the host, and every entry
// below draws the token that restatement draws (tests/test_gpu_draw_exact.py).
#include "common.h"
#include "internal.h"
#include "pick.h"

namespace {

constexpr int SMP_LIST = 256;  // kept-set capacity: top_k plus ties at the k-th score

__device__ __forceinline__ unsigned key_of(float s) {
  const unsigned u = __float_as_uint(s);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);  // unsigned order == float order (-inf .. +inf)
}
__device__ __forceinline__ float score_of(unsigned k) {
  return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k);
}

// k-th largest (k = 1 .. n) of keys[0 .. n) held in LDS; every thread of the block calls it (barriers inside).
// Returns the key; *need_eq = how many entries EQUAL to it belong to the top k, *count_eq = how many such entries exist.
struct SelectLds {
  unsigned hist[256];
  unsigned bin, above, cnt;
};
__device__ unsigned block_select_kth(const unsigned* __restrict__ keys, int n, int k, SelectLds& L, int* need_eq, int* count_eq) {
  const int tid = threadIdx.x, nt = blockDim.x, lane = tid & 63;
  unsigned prefix = 0, mask = 0;
  int remaining = k;
  unsigned last_cnt = 0;
#pragma unroll 1
  for (int pass = 0; pass < 4; ++pass) {
    const int shift = 24 - 8 * pass;
    if (tid < 256) L.hist[tid] = 0;
    __syncthreads();
    for (int i = tid; i < n; i += nt) {
      const unsigned key = keys[i];
      if ((key & mask) == prefix) atomicAdd(&L.hist[(key >> shift) & 255u], 1u);
    }
    __syncthreads();
    if (tid < 64) {  // one wave: suffix sums over the 256 bins, 4 bins per lane
      const unsigned c0 = L.hist[4 * lane], c1 = L.hist[4 * lane + 1], c2 = L.hist[4 * lane + 2], c3 = L.hist[4 * lane + 3];
      const unsigned tot = c0 + c1 + c2 + c3;
      unsigned v = tot;  // inclusive suffix over lanes
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const unsigned t = __shfl_down(v, o);
        if (lane + o < 64) v += t;
      }
      const unsigned e = v - tot;  // entries in bins above this lane's four
      const unsigned s3 = e + c3, s2 = s3 + c2, s1 = s2 + c1, s0 = s1 + c0;
      const unsigned need = (unsigned)remaining;
      // exactly one (lane, j): S[bin] >= need > S[bin + 1]
      if (s3 >= need && e < need) { L.bin = 4 * lane + 3; L.above = e; L.cnt = c3; }
      else if (s2 >= need && s3 < need) { L.bin = 4 * lane + 2; L.above = s3; L.cnt = c2; }
      else if (s1 >= need && s2 < need) { L.bin = 4 * lane + 1; L.above = s2; L.cnt = c1; }
      else if (s0 >= need && s1 < need) { L.bin = 4 * lane; L.above = s1; L.cnt = c0; }
    }
    __syncthreads();
    prefix |= L.bin << shift;
    mask |= 0xFFu << shift;
    remaining -= (int)L.above;
    last_cnt = L.cnt;
    __syncthreads();
  }
  *need_eq = remaining;
  *count_eq = (int)last_cnt;
  return prefix;
}

// MODE (every sampler kernel below): how row b addresses the Philox stream (PickRows / pick_draw, pick.h) -- the rows are sequences of
// one step, successive steps of ONE sequence (the lookup step's T rows), or B sequences x T steps (the batched lookup step's rows; only
// then SEQS is one PickSeqs, otherwise the pack is empty and the kernel has the arguments it always had).  Nothing else differs.
template <PickRows MODE, class... SEQS>
__global__ __launch_bounds__(256) void sample_partial_kernel(const float* __restrict__ logits, const srgpt_sampling* __restrict__ sp,
                                                             unsigned* __restrict__ cand_key, int* __restrict__ cand_idx,
                                                             float* __restrict__ pv, int* __restrict__ pi, int V, SEQS... seqs) {
  __shared__ unsigned keys[PICK_SLICE_MAX];
  __shared__ SelectLds L;
  __shared__ unsigned cnt;
  const int b = blockIdx.y, nb = gridDim.x, blk = blockIdx.x, tid = threadIdx.x;
  const PickSlice sl = pick_slice(V);
  const int lo = sl.lo, hi = sl.hi, n = max(hi - lo, 0);
  const float* row = logits + (size_t)b * V;
  const float T = sp->temperature;
  const int topk = min(sp->top_k, SMP_K);
  if (topk <= 0) {
    // ---- Gumbel-max over logits / T: the slice's best key for the greedy merge ----
    const PickDraw dr = pick_draw<MODE>(sp->counter, b, seqs...);
    const unsigned long long seed = sp->seed;
    float best = -INFINITY;
    int bi = PICK_NONE;
    for (int i = lo + tid; i < hi; i += 256) {
      const float v = pick_gumbel_key(row[i] / T, dr.ctr, seed, dr.seq, i);
      if (v > best) {
        best = v;
        bi = i;
      }
    }
    pick_store_slice(best, bi, pv, pi);
    return;
  }
  // ---- top-k of the slice ----
  const size_t base = ((size_t)b * nb + blk) * SMP_K;
  if (tid < SMP_K) {
    cand_key[base + tid] = 0u;  // below every real key
    cand_idx[base + tid] = -1;
  }
  if (tid == 0) cnt = 0;
  for (int i = tid; i < n; i += 256) keys[i] = key_of(row[lo + i] / T);
  __syncthreads();
  if (n == 0) return;  // uniform
  const int kk = min(topk, n);
  int need_eq, count_eq;
  const unsigned thr = block_select_kth(keys, n, kk, L, &need_eq, &count_eq);
  // everything above the slice's k-th score, and EVERY entry equal to it while the 64 slots last: TopKLogitsWarper keeps ties at the
  // global k-th score, so a slice must not drop its share of them (three equal maxima in one slice under top_k = 1 are three kept
  // tokens).  Only a slice with more than 64 - (entries above) equal scores truncates -- lowest indices first, a fixed set.
  const int room = SMP_K - (kk - need_eq);
  for (int i = tid; i < n; i += 256) {
    const unsigned key = keys[i];
    bool take = key > thr;
    if (key == thr) {
      if (count_eq <= room) take = true;
      else {
        int r = 0;
        for (int j = 0; j < i; ++j) r += keys[j] == thr;
        take = r < room;
      }
    }
    if (take) {
      const unsigned slot = atomicAdd(&cnt, 1u);
      if (slot < (unsigned)SMP_K) {
        cand_key[base + slot] = key;
        cand_idx[base + slot] = lo + i;
      }
    }
  }
}

template <PickRows MODE, class... SEQS>
__global__ __launch_bounds__(1024) void sample_select_kernel(const srgpt_sampling* __restrict__ sp, const unsigned* __restrict__ cand_key,
                                                             const int* __restrict__ cand_idx, int64_t* __restrict__ tok, int nb,
                                                             int* __restrict__ err, SEQS... seqs) {
  constexpr int NC = PICK_SLICES * SMP_K;
  __shared__ unsigned keys[NC];
  __shared__ int idxs[NC];
  __shared__ SelectLds L;
  __shared__ unsigned lkey[SMP_LIST];
  __shared__ int lidx[SMP_LIST];
  __shared__ float ss[SMP_LIST];
  __shared__ int sidx[SMP_LIST];
  __shared__ unsigned n_valid, n_list;
  // settings the device sampler does not serve must not draw from a silently different distribution: top_k beyond the
  // candidate slots would be clamped, and a top-p filter without top-k would be ignored by the Gumbel path -- error bit 4, reported
  // by srgpt_llm_decode_sync_state (the state's word: sticky) / srgpt_sample_status (the workspace's word: the last srgpt_sample call)
  if (blockIdx.x == 0 && threadIdx.x == 0 && (sp->top_k > SMP_K || (sp->top_k <= 0 && sp->top_p < 1.f))) atomicOr(err, 4);
  const int topk = min(sp->top_k, SMP_K);
  if (topk <= 0) return;  // Gumbel-max mode: the greedy merge (advance_kernel) picks
  const int b = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
  const int n = nb * SMP_K;
  if (tid == 0) {
    n_valid = 0;
    n_list = 0;
  }
  __syncthreads();
  unsigned mine = 0;
  for (int i = tid; i < n; i += nt) {
    const int ix = cand_idx[(size_t)b * n + i];
    keys[i] = cand_key[(size_t)b * n + i];
    idxs[i] = ix;
    mine += ix >= 0;
  }
  if (mine) atomicAdd(&n_valid, mine);
  __syncthreads();
  const int kk = min(topk, (int)n_valid);
  if (kk <= 0) {  // no vocabulary at all: cannot happen for V >= 1
    if (tid == 0) tok[b] = 0;
    return;
  }
  int need_eq, count_eq;
  const unsigned thr = block_select_kth(keys, n, kk, L, &need_eq, &count_eq);
  for (int i = tid; i < n; i += nt)
    if (idxs[i] >= 0 && keys[i] >= thr) {
      const unsigned slot = atomicAdd(&n_list, 1u);
      if (slot < (unsigned)SMP_LIST) {
        lkey[slot] = keys[i];
        lidx[slot] = idxs[i];
      }
    }
  __syncthreads();
  if (n_list > (unsigned)SMP_LIST && tid == 0) atomicOr(err, 2);  // > 256 - k entries tie at the k-th score: reported, not silent
  const int nk = min((int)n_list, SMP_LIST);
  // rank by (score desc, index DESC): TopPLogitsWarper sorts ascending and cuts from the small end, never the last entry.  Where the
  // cut runs through a group of exactly equal scores, which members survive is torch.sort's tie order -- index order for short
  // rows (then the HIGHEST index survives longest: what this order reproduces), unspecified for long ones -- so only the kept
  // VALUES are defined there.  A total order: the list does not depend on the append order above.
  for (int e = tid; e < nk; e += nt) {
    const unsigned ke = lkey[e];
    const int ie = lidx[e];
    int r = 0;
    for (int j = 0; j < nk; ++j) r += (lkey[j] > ke) || (lkey[j] == ke && lidx[j] > ie);
    ss[r] = score_of(ke);
    sidx[r] = ie;
  }
  __syncthreads();
  if (tid == 0) {
    const float m = ss[0];
    int n2 = nk;
    const float top_p = sp->top_p;
    if (top_p < 1.0f) {
      // TopPLogitsWarper: sort ascending, softmax, cumulative sum; remove while cumsum <= 1 - top_p, never the last (largest)
      float Z = 0.f;
      for (int r = nk - 1; r >= 0; --r) Z += __expf(ss[r] - m);
      float c = 0.f;
      for (int r = nk - 1; r >= 1; --r) {
        c += __expf(ss[r] - m) / Z;
        if (c <= sp->top_p_rm) n2 = r;
        else break;
      }
    }
    float Z2 = 0.f;
    for (int r = 0; r < n2; ++r) Z2 += __expf(ss[r] - m);
    const PickDraw dr = pick_draw<MODE>(sp->counter, b, seqs...);
    const unsigned long long ctr = dr.ctr, seed = sp->seed;
    const U4 rr = philox4x32_10(U4{(unsigned)ctr, (unsigned)(ctr >> 32), (unsigned)dr.seq, 0xFFFFFFFFu}, (unsigned)seed, (unsigned)(seed >> 32));
    const float u = (float)(rr.x >> 8) * (1.0f / 16777216.0f);  // [0, 1)
    const float target = u * Z2;
    int pick = n2 - 1;
    float c = 0.f;
    for (int r = 0; r < n2; ++r) {
      c += __expf(ss[r] - m);
      if (target < c) {
        pick = r;
        break;
      }
    }
    tok[b] = sidx[pick];
    int* ko = sp->kept_out;
    if (ko) {  // parity hook: the kept set of this step, best first
      ko += (size_t)b * (SMP_LIST + 1);
      ko[0] = n2;
      for (int r = 0; r < n2; ++r) ko[1 + r] = sidx[r];
    }
  }
}

// the stand-alone ops only (the decode step's advance_kernel does both): merge the slices' maxima, one wave per row -- always (the full
// sampler), or only in Gumbel mode (srgpt_sample: sample_select_kernel drew the token otherwise); every call advances the counter --
// by one step, or (PICK_ROWS_STEPS: the B rows were B steps) by B -- but for rows of several sequences (PICK_ROWS_SEQ_STEPS, SP =
// const srgpt_sampling): how far those advance is their accept's decision, the block is only read
template <PickRows MODE, class SP>
__global__ void sample_merge_kernel(SP* sp, const float* __restrict__ pv, const int* __restrict__ pi, int64_t* __restrict__ tok, int B,
                                    int always) {
  if (always || sp->top_k <= 0)
    for (int b = threadIdx.x >> 6; b < B; b += blockDim.x >> 6) {
      const int t = pick_merge_row(pv + (size_t)b * PICK_SLICES, pi + (size_t)b * PICK_SLICES, PICK_SLICES, threadIdx.x & 63);
      if ((threadIdx.x & 63) == 0) tok[b] = t;
    }
  if constexpr (MODE != PICK_ROWS_SEQ_STEPS) {
    __syncthreads();
    if (threadIdx.x == 0) sp->counter += MODE == PICK_ROWS_STEPS ? (unsigned long long)B : 1ull;
  }
}

// ================================================================================================
// The full sampler: every temperature / top_k / top_p over the whole vocabulary.  The kept set is always a SUFFIX of the row in
// the order (score asc, index asc): top-k removes every key below the k-th largest (ties kept), top-p then removes a prefix of that
// order (HF's ascending sort; CPU torch.sort puts the lower index of equal scores first).  So one (key, index) pair per row says
// everything: kept <=> key > tkey || (key == tkey && index >= tidx).
// ================================================================================================
constexpr int SFU_THREADS = 1024;
constexpr int SFU_BINS = 4096;  // digits of a 32-bit key: 12 + 10 + 10 bits
constexpr float SFU_FIX = 35184372088832.0f;  // 2^45: mass exp(s - max) in (0, 1] as 64-bit fixed point; V <= 2^18 entries sum < 2^63

struct FullLds {
  unsigned long long hist[SFU_BINS];
  unsigned long long part[SFU_THREADS / 64];
  unsigned long long below, in_bin;
  unsigned bin, maxkey;
};

__device__ __forceinline__ unsigned long long mass_of(unsigned key, float m) { return __float2ull_rn(expf(score_of(key) - m) * SFU_FIX); }

// digit `level` of a key: bits 31..20, 19..10, 9..0; the bits above it must equal the prefix found so far
__device__ __forceinline__ int digit_shift(int level) { return level == 0 ? 20 : (level == 1 ? 10 : 0); }
__device__ __forceinline__ unsigned digit_bins(int level) { return level == 0 ? 4096u : 1024u; }
__device__ __forceinline__ unsigned above_mask(int level) { return level == 0 ? 0u : (level == 1 ? 0xFFF00000u : 0xFFFFFC00u); }

// f(key, i) for every entry of the row, thread tid taking i = tid + j * 1024 (the entries it wrote in pass 0); 8 independent loads in
// flight per thread (one at a time, a pass over 128k L2-resident keys was ~40 us of load latency)
constexpr int SFU_UNROLL = 8;
template <class F>
__device__ __forceinline__ void for_keys(const unsigned* __restrict__ keys, int V, F f) {
  for (int i0 = threadIdx.x; i0 < V; i0 += SFU_THREADS * SFU_UNROLL) {
    unsigned k[SFU_UNROLL];
#pragma unroll
    for (int u = 0; u < SFU_UNROLL; ++u) k[u] = keys[min(i0 + u * SFU_THREADS, V - 1)];
#pragma unroll
    for (int u = 0; u < SFU_UNROLL; ++u)
      if (i0 + u * SFU_THREADS < V) f(k[u], i0 + u * SFU_THREADS);
  }
}

__device__ void clear_hist(FullLds& L, int nbins) {
  for (int i = threadIdx.x; i < nbins; i += SFU_THREADS) L.hist[i] = 0;
  __syncthreads();
}

// the smallest bin d whose inclusive prefix P(d) over hist[0 .. nbins) exceeds X (the total must exceed X): L.bin = d,
// L.below = P(d - 1), L.in_bin = hist[d].  Integer sums in a fixed order: the same answer on every replay.
__device__ void find_bin(FullLds& L, int nbins, unsigned long long X) {
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, per = nbins / SFU_THREADS;
  unsigned long long s = 0;
  for (int j = 0; j < per; ++j) s += L.hist[tid * per + j];
  unsigned long long v = s;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned long long t = __shfl_up(v, o);
    if (lane >= o) v += t;
  }
  if (lane == 63) L.part[wv] = v;
  __syncthreads();
  unsigned long long run = v - s;
  for (int w = 0; w < wv; ++w) run += L.part[w];
  for (int j = 0; j < per; ++j) {
    const unsigned long long h = L.hist[tid * per + j];
    if (run <= X && X < run + h) {
      L.bin = tid * per + j;
      L.below = run;
      L.in_bin = h;
    }
    run += h;
  }
  __syncthreads();
}

__device__ unsigned long long hist_total(FullLds& L, int nbins) {
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  unsigned long long s = 0;
  for (int i = tid; i < nbins; i += SFU_THREADS) s += L.hist[i];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
  if (lane == 0) L.part[wv] = s;
  __syncthreads();
  unsigned long long t = 0;
  for (int w = 0; w < SFU_THREADS / 64; ++w) t += L.part[w];
  __syncthreads();
  return t;
}

// launch 1 of the full sampler: one block per sequence finds the row's threshold pair (tkey, tidx).  Pass 0 writes the order-preserving
// keys of logits / T to the workspace (each thread later re-reads only the entries it wrote) and takes the maximum; top-k is a 3-digit
// radix select by counts, top-p the same digit walk by fixed-point softmax mass over the top-k survivors, and where the top-p cut runs
// through a group of equal scores a 2-digit select over their indices says how many of them (lowest indices first) go.
// (No STEPS mode: the kernel reads no random number, so rows that are steps and rows that are sequences are the same launch.  As a
// template its <false> instantiation came out with two registers renamed; it stays a plain kernel and keeps its machine code.)
__global__ __launch_bounds__(SFU_THREADS) void sample_full_threshold_kernel(const float* __restrict__ logits,
                                                                          const srgpt_sampling* __restrict__ sp,
                                                                          unsigned* __restrict__ keys_ws, unsigned* __restrict__ thr,
                                                                          int V) {
  __shared__ FullLds L;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
  const float* row = logits + (size_t)b * V;
  unsigned* keys = keys_ws + (size_t)b * V;
  const float T = sp->temperature;
  const int top_k = sp->top_k;
  const bool p_on = sp->top_p < 1.0f;
  const int k = top_k != 0 ? min(max(top_k, 1), V) : V;  // TopKLogitsWarper: min(max(top_k, min_tokens_to_keep), V)
  const bool k_on = k < V;
  if (tid == 0) L.maxkey = 0;
  clear_hist(L, SFU_BINS);
  unsigned mx = 0;
  for (int i0 = tid; i0 < V; i0 += SFU_THREADS * SFU_UNROLL) {
    float x[SFU_UNROLL];
#pragma unroll
    for (int u = 0; u < SFU_UNROLL; ++u) x[u] = row[min(i0 + u * SFU_THREADS, V - 1)];
#pragma unroll
    for (int u = 0; u < SFU_UNROLL; ++u) {
      const int i = i0 + u * SFU_THREADS;
      if (i < V) {
        const unsigned key = key_of(x[u] / T);  // a true division, as HF's TemperatureLogitsWarper
        keys[i] = key;
        mx = max(mx, key);
        if (k_on) atomicAdd(&L.hist[key >> 20], 1ull);
      }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mx = max(mx, (unsigned)__shfl_xor(mx, o));
  if (lane == 0) atomicMax(&L.maxkey, mx);
  __syncthreads();
  const unsigned maxkey = L.maxkey;

  // ---- top-k: the k-th largest key = the smallest key t with #(keys <= t) > V - k ----
  unsigned kthr = 0;
  if (k_on) {
    unsigned prefix = 0;
    unsigned long long X = (unsigned long long)(V - k);
#pragma unroll 1
    for (int level = 0; level < 3; ++level) {
      const int sh = digit_shift(level);
      const unsigned nb = digit_bins(level), am = above_mask(level);
      if (level > 0) {
        clear_hist(L, SFU_THREADS);
        for_keys(keys, V, [&](unsigned key, int) {
          if ((key & am) == prefix) atomicAdd(&L.hist[(key >> sh) & (nb - 1)], 1ull);
        });
        __syncthreads();
      }
      find_bin(L, (int)max(nb, (unsigned)SFU_THREADS), X);
      prefix |= L.bin << sh;
      X -= L.below;
      __syncthreads();
    }
    kthr = prefix;
  }

  unsigned tkey = kthr, tidx = 0;
  if (p_on) {
    // ---- top-p over the survivors (key >= kthr): cumulative mass in (score asc, index asc) order; an entry goes while its
    // cumulative mass S <= top_p_rm * Z.  The first survivor is the smallest key t with S(keys <= t) > R = floor(top_p_rm * Z),
    // R clamped below Z: the largest entry always stays (top_p = 0 keeps exactly one) ----
    const float m = score_of(maxkey);
    unsigned prefix = 0;
    unsigned long long X = 0, R = 0;
#pragma unroll 1
    for (int level = 0; level < 3; ++level) {
      const int sh = digit_shift(level);
      const unsigned nb = digit_bins(level), am = above_mask(level);
      clear_hist(L, (int)nb);
      for_keys(keys, V, [&](unsigned key, int) {
        if (key >= kthr && (key & am) == prefix) atomicAdd(&L.hist[(key >> sh) & (nb - 1)], mass_of(key, m));
      });
      __syncthreads();
      if (level == 0) {
        const unsigned long long Z = hist_total(L, SFU_BINS);
        R = (unsigned long long)((double)Z * (double)sp->top_p_rm);
        if (R >= Z) R = Z - 1;
        X = R;
      }
      find_bin(L, (int)max(nb, (unsigned)SFU_THREADS), X);
      prefix |= L.bin << sh;
      X -= L.below;
      __syncthreads();
    }
    tkey = prefix;
    // every entry of key tkey carries the same mass q: the j-th of them (ascending index) has S = S(keys < tkey) + j q, so the
    // r = X / q lowest indices go
    const unsigned long long q = mass_of(tkey, m);
    const unsigned long long r = X / q;
    if (r > 0) {
      // the (r + 1)-th smallest index among the entries of key tkey: V <= 2^18, digits idx >> 8 (<= 1024 bins) and idx & 255
      unsigned ip = 0;
      unsigned long long Xi = r;
#pragma unroll 1
      for (int level = 0; level < 2; ++level) {
        clear_hist(L, SFU_THREADS);
        for_keys(keys, V, [&](unsigned key, int i) {
          if (key == tkey && (level == 0 || (unsigned)(i >> 8) == ip)) atomicAdd(&L.hist[level == 0 ? (i >> 8) : (i & 255)], 1ull);
        });
        __syncthreads();
        find_bin(L, SFU_THREADS, Xi);
        ip = level == 0 ? L.bin : ((ip << 8) | L.bin);
        Xi -= L.below;
        __syncthreads();
      }
      tidx = ip;
    }
  }
  if (tid == 0) {
    thr[(size_t)b * 4] = tkey;
    thr[(size_t)b * 4 + 1] = tidx;
  }
}

// launch 2: masked Gumbel-max per vocabulary slice, grid (PICK_SLICES, batch) -> the per-slice (value, index) pairs the greedy merge
// (advance_kernel, or sample_merge_kernel for the stand-alone op) consumes.  Same Philox addressing as the top_k = 0 path of
// sample_partial_kernel.  kept_mask (optional): bit i % 32 of word i / 32 of the row = entry i kept.
template <PickRows MODE, class... SEQS>
__global__ __launch_bounds__(256) void sample_full_draw_kernel(const srgpt_sampling* __restrict__ sp, const unsigned* __restrict__ keys_ws,
                                                              const unsigned* __restrict__ thr, float* __restrict__ pv,
                                                              int* __restrict__ pi, unsigned* __restrict__ kept_mask, int V, SEQS... seqs) {
  const int b = blockIdx.y, nb = gridDim.x, blk = blockIdx.x, tid = threadIdx.x;
  const PickSlice sl = pick_slice(V);
  const unsigned* keys = keys_ws + (size_t)b * V;
  const unsigned tkey = thr[(size_t)b * 4], tidx = thr[(size_t)b * 4 + 1];
  const PickDraw dr = pick_draw<MODE>(sp->counter, b, seqs...);
  const unsigned long long seed = sp->seed;
  float best = -INFINITY;
  int bi = PICK_NONE;
  for (int i = sl.lo + tid; i < sl.hi; i += 256) {
    const unsigned key = keys[i];
    if (key < tkey || (key == tkey && (unsigned)i < tidx)) continue;
    const float v = pick_gumbel_key(score_of(key), dr.ctr, seed, dr.seq, i);
    if (v > best) {
      best = v;
      bi = i;
    }
  }
  pick_store_slice(best, bi, pv, pi);
  if (kept_mask) {
    const int nw = (V + 31) / 32;
    for (int w = blk * 256 + tid; w < nw; w += nb * 256) {
      unsigned bits = 0;
      for (int j = 0; j < 32; ++j) {
        const int i = w * 32 + j;
        if (i >= V) break;
        const unsigned key = keys[i];
        if (key > tkey || (key == tkey && (unsigned)i >= tidx)) bits |= 1u << j;
      }
      kept_mask[(size_t)b * nw + w] = bits;
    }
  }
}

}  // namespace

// the top-k-64 sampler's workspace (SampleWs, pick.h)
extern "C" int64_t srgpt_sample_ws_bytes(int B) { return B <= 0 ? -1 : carve_sample_ws(nullptr, B).bytes; }

// launches 1 and 2 of the top-k-64 sampler over B rows: sequences, successive steps of one sequence, or (seqs: one PickSeqs) the
// rows of seqs.B sequences x seqs.T steps
template <PickRows MODE, class... SEQS>
static int sample_launch(const float* logits, const srgpt_sampling* sp, int64_t* tok, void* ws, float* pv, int* pi, int* err, int B, int V,
                         hipStream_t s, SEQS... seqs) {
  SRGPT_CHECK(logits && sp && tok && ws && pv && pi && err, SRGPT_ERR_ARG, "srgpt_sample: null pointer");
  SRGPT_CHECK(B > 0 && V > 0, SRGPT_ERR_UNSUPPORTED, "srgpt_sample: empty shape");
  SRGPT_TRY(pick_check_vocab(V, "srgpt_sample"));
  const SampleWs c = carve_sample_ws(ws, B);
  hipLaunchKernelGGL((sample_partial_kernel<MODE, SEQS...>), dim3(PICK_SLICES, B), dim3(256), 0, s, logits, sp, c.cand_key, c.cand_idx, pv,
                     pi, V, seqs...);
  hipLaunchKernelGGL((sample_select_kernel<MODE, SEQS...>), dim3(B), dim3(1024), 0, s, sp, c.cand_key, c.cand_idx, tok, PICK_SLICES, err,
                     seqs...);
  SRGPT_LAUNCH_CHECK();
  return SRGPT_OK;
}

// internal (model.hip): launches 1 and 2; the caller books the token (advance_kernel) and advances the counter
int srgpt_sample_launch(const float* logits, const srgpt_sampling* sp, int64_t* tok, void* ws, float* pv, int* pi, int* err, int B, int V,
                        hipStream_t s) {
  return sample_launch<PICK_ROWS_SEQS>(logits, sp, tok, ws, pv, pi, err, B, V, s);
}

// internal (model.hip, the sampled lookup step): the same over T rows that are successive steps of one sequence -- row t draws at
// counter + t; the caller accepts (lookup.hip) and advances the counter by what it emitted
int srgpt_sample_rows_launch(const float* logits, const srgpt_sampling* sp, int64_t* tok, void* ws, float* pv, int* pi, int* err, int T,
                             int V, hipStream_t s) {
  return sample_launch<PICK_ROWS_STEPS>(logits, sp, tok, ws, pv, pi, err, T, V, s);
}

// internal (model.hip, the batched sampled lookup step): the same over the B * T rows of B sequences x T steps -- row b * T + t draws
// at draw_addr.h's address over steps [B] (device); the caller accepts (lookup.hip) and moves the counter with the filled column
int srgpt_sample_seq_rows_launch(const float* logits, const srgpt_sampling* sp, const int* steps, int64_t* tok, void* ws, float* pv, int* pi,
                                 int* err, int B, int T, int V, hipStream_t s) {
  SRGPT_CHECK(steps && B > 0 && T > 0, SRGPT_ERR_ARG, "srgpt_sample_seq_rows: null steps or empty shape");
  return sample_launch<PICK_ROWS_SEQ_STEPS>(logits, sp, tok, ws, pv, pi, err, B * T, V, s, PickSeqs{steps, B, T});
}

// the stand-alone draw: clear the workspace's error word, launches 1 and 2, the Gumbel-mode merge and (SP not const) the counter
template <PickRows MODE, class SP, class... SEQS>
static int sample_op(const float* logits, SP* sp, int64_t* tok_out, void* ws, int B, int V, srgpt_stream_t stream, SEQS... seqs) {
  SRGPT_CHECK(logits && sp && tok_out && ws && B > 0 && V > 0, SRGPT_ERR_ARG, "srgpt_sample: null pointer or empty shape");
  SRGPT_TRY(pick_check_vocab(V, "srgpt_sample"));
  const SampleWs c = carve_sample_ws(ws, B);
  hipStream_t s = as_stream(stream);
  SRGPT_HIP_TRY(hipMemsetAsync(c.err, 0, sizeof(int), s), "srgpt_sample: clearing the error word");
  SRGPT_TRY(sample_launch<MODE>(logits, sp, tok_out, ws, c.pv, c.pi, c.err, B, V, s, seqs...));
  hipLaunchKernelGGL((sample_merge_kernel<MODE, SP>), dim3(1), dim3(256), 0, s, sp, c.pv, c.pi, tok_out, B, 0);
  SRGPT_LAUNCH_CHECK();
  return SRGPT_OK;
}

extern "C" int srgpt_sample(const float* logits, srgpt_sampling* sp, int64_t* tok_out, void* ws, int B, int V, srgpt_stream_t stream) {
  return sample_op<PICK_ROWS_SEQS>(logits, sp, tok_out, ws, B, V, stream);
}

extern "C" int srgpt_sample_rows(const float* logits, srgpt_sampling* sp, int64_t* tok_out, void* ws, int T, int V, srgpt_stream_t stream) {
  return sample_op<PICK_ROWS_STEPS>(logits, sp, tok_out, ws, T, V, stream);
}

// both stand-alone entries over B sequences x T steps: the sizes, before anything else is looked at
static int check_seq_rows(const int* steps, int B, int T, int V, const char* fn) {
  SRGPT_CHECK(steps, SRGPT_ERR_ARG, "%s: null pointer", fn);
  SRGPT_CHECK(B >= 1 && T >= 1 && V >= 1 && (int64_t)B * T <= INT_MAX, SRGPT_ERR_ARG, "%s: bad sizes B=%d T=%d V=%d", fn, B, T, V);
  return SRGPT_OK;
}

extern "C" int srgpt_sample_seq_rows(const float* logits, const srgpt_sampling* sp, const int* steps, int64_t* tok_out, void* ws, int B,
                                     int T, int V, srgpt_stream_t stream) {
  SRGPT_TRY(check_seq_rows(steps, B, T, V, "srgpt_sample_seq_rows"));
  return sample_op<PICK_ROWS_SEQ_STEPS>(logits, sp, tok_out, ws, B * T, V, stream, PickSeqs{steps, B, T});
}

// health of the last srgpt_sample call(s) on this workspace (synchronises `stream`): the sticky error word at the tail of ws
extern "C" int srgpt_sample_status(const void* ws, int B, srgpt_stream_t stream) {
  SRGPT_CHECK(ws && B > 0, SRGPT_ERR_ARG, "srgpt_sample_status: bad args");
  int host = 0;
  SRGPT_HIP_TRY(hipMemcpyAsync(&host, carve_sample_ws(ws, B).err, sizeof(int), hipMemcpyDeviceToHost, as_stream(stream)), "srgpt_sample_status: copy");
  SRGPT_HIP_TRY(hipStreamSynchronize(as_stream(stream)), "srgpt_sample_status: synchronize");
  SRGPT_CHECK((host & 4) == 0, SRGPT_ERR_UNSUPPORTED,
              "sampling: top_k > %d, or a top-p filter without top-k, is not served by the device sampler (the draw used another distribution)", SMP_K);
  SRGPT_CHECK((host & 2) == 0, SRGPT_ERR_STATE, "sampling: more than %d vocabulary entries tie at the top-k threshold (kept set truncated)", SMP_LIST);
  return SRGPT_OK;
}

// ---- the full sampler: its workspace is SampleFullWs (pick.h) ----
extern "C" int64_t srgpt_sample_full_ws_bytes(int B, int V) { return B <= 0 || V <= 0 ? -1 : carve_sample_full_ws(nullptr, B, V).bytes; }

template <PickRows MODE, class... SEQS>
static int sample_full_launch(const float* logits, const srgpt_sampling* sp, void* keys_thr, float* pv, int* pi, unsigned* kept_mask, int B,
                              int V, hipStream_t s, SEQS... seqs) {
  SRGPT_CHECK(logits && sp && keys_thr && pv && pi, SRGPT_ERR_ARG, "srgpt_sample_full: null pointer");
  SRGPT_CHECK(B > 0 && V > 0, SRGPT_ERR_ARG, "srgpt_sample_full: empty shape");
  SRGPT_TRY(pick_check_vocab(V, "srgpt_sample_full"));
  const SampleFullWs c = carve_sample_full_ws(keys_thr, B, V);
  hipLaunchKernelGGL(sample_full_threshold_kernel, dim3(B), dim3(SFU_THREADS), 0, s, logits, sp, c.keys, c.thr, V);
  hipLaunchKernelGGL((sample_full_draw_kernel<MODE, SEQS...>), dim3(PICK_SLICES, B), dim3(256), 0, s, sp, c.keys, c.thr, pv, pi, kept_mask,
                     V, seqs...);
  SRGPT_LAUNCH_CHECK();
  return SRGPT_OK;
}

// internal (model.hip): launches 1 and 2 into the caller's slice maxima pv / pi ([B][128]); the caller merges, books the token and
// advances the counter.  keys_thr = the head (keys and thresholds) of a SampleFullWs.
int srgpt_sample_full_launch(const float* logits, const srgpt_sampling* sp, void* keys_thr, float* pv, int* pi, unsigned* kept_mask, int B,
                             int V, hipStream_t s) {
  return sample_full_launch<PICK_ROWS_SEQS>(logits, sp, keys_thr, pv, pi, kept_mask, B, V, s);
}

// internal (model.hip, the sampled lookup step): the same over T rows that are successive steps of one sequence
int srgpt_sample_full_rows_launch(const float* logits, const srgpt_sampling* sp, void* keys_thr, float* pv, int* pi, unsigned* kept_mask,
                                  int T, int V, hipStream_t s) {
  return sample_full_launch<PICK_ROWS_STEPS>(logits, sp, keys_thr, pv, pi, kept_mask, T, V, s);
}

// internal (model.hip, the batched sampled lookup step): the same over the B * T rows of B sequences x T steps (steps [B], device)
int srgpt_sample_full_seq_rows_launch(const float* logits, const srgpt_sampling* sp, const int* steps, void* keys_thr, float* pv, int* pi,
                                      unsigned* kept_mask, int B, int T, int V, hipStream_t s) {
  SRGPT_CHECK(steps && B > 0 && T > 0, SRGPT_ERR_ARG, "srgpt_sample_full_seq_rows: null steps or empty shape");
  return sample_full_launch<PICK_ROWS_SEQ_STEPS>(logits, sp, keys_thr, pv, pi, kept_mask, B * T, V, s, PickSeqs{steps, B, T});
}

template <PickRows MODE, class SP, class... SEQS>
static int sample_full_op(const float* logits, SP* sp, int64_t* tok_out, uint32_t* kept_mask, void* ws, int B, int V, srgpt_stream_t stream,
                          SEQS... seqs) {
  SRGPT_CHECK(tok_out && ws, SRGPT_ERR_ARG, "srgpt_sample_full: null pointer");
  SRGPT_CHECK(B > 0 && V > 0, SRGPT_ERR_ARG, "srgpt_sample_full: empty shape");
  const SampleFullWs c = carve_sample_full_ws(ws, B, V);
  hipStream_t s = as_stream(stream);
  SRGPT_TRY(sample_full_launch<MODE>(logits, sp, ws, c.pv, c.pi, reinterpret_cast<unsigned*>(kept_mask), B, V, s, seqs...));
  hipLaunchKernelGGL((sample_merge_kernel<MODE, SP>), dim3(1), dim3(256), 0, s, sp, c.pv, c.pi, tok_out, B, 1);
  SRGPT_LAUNCH_CHECK();
  return SRGPT_OK;
}

extern "C" int srgpt_sample_full(const float* logits, srgpt_sampling* sp, int64_t* tok_out, uint32_t* kept_mask, void* ws, int B, int V,
                                 srgpt_stream_t stream) {
  return sample_full_op<PICK_ROWS_SEQS>(logits, sp, tok_out, kept_mask, ws, B, V, stream);
}

extern "C" int srgpt_sample_full_rows(const float* logits, srgpt_sampling* sp, int64_t* tok_out, uint32_t* kept_mask, void* ws, int T, int V,
                                      srgpt_stream_t stream) {
  return sample_full_op<PICK_ROWS_STEPS>(logits, sp, tok_out, kept_mask, ws, T, V, stream);
}

extern "C" int srgpt_sample_full_seq_rows(const float* logits, const srgpt_sampling* sp, const int* steps, int64_t* tok_out,
                                          uint32_t* kept_mask, void* ws, int B, int T, int V, srgpt_stream_t stream) {
  SRGPT_TRY(check_seq_rows(steps, B, T, V, "srgpt_sample_full_seq_rows"));
  return sample_full_op<PICK_ROWS_SEQ_STEPS>(logits, sp, tok_out, kept_mask, ws, B * T, V, stream, PickSeqs{steps, B, T});
}
