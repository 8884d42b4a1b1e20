// Which attention kernel a call runs on, with which template arguments and launch shape, and where the decode kernels keep their
// partials: the host-side selection of attn.hip / flash.hip as pure functions of the shape and the CU count, plus the one description
// of the decode workspace that host and device share.  Plain C++ (no HIP; what device code calls is constexpr):
// tests/test_host_attn_route.py compiles this header alone and pins the launch of every attention call of the models
// (tests/golden/attn_routes.json) -- every threshold below was calibrated on the MI355X, and all routes compute the same result
// within tolerance, so nothing else notices a slipped comparison.
#pragma once
#include <stddef.h>
#include <stdint.h>

enum AttnFamily {
  ATTN_FLASH,        // flash_bf16_kernel<HDP, CAUSAL> (flash.hip): MFMA, bf16, 64 query rows per 4-wave block
  ATTN_ONE_WAVE,     // simple_attn_kernel<T> (attn.hip): one wave per (query row, head); any dtype / head_dim; fp32 parity path
  ATTN_DECODE_MFMA,  // decode_mfma_kernel<G> (attn.hip): bf16, head_dim 128, fixed key ranges of kpb keys per block
  ATTN_DECODE_VALU,  // decode_split_kernel<T, D, G> (attn.hip): the sequence's keys cut evenly into nsplit chunks
  ATTN_DECODE_MULTI_MFMA,      // decode_mfma_multi_kernel<NC> (attn.hip): T new tokens per sequence in the B operand's 16 columns
  ATTN_DECODE_MULTI_COMPOSED,  // srgpt_decode_attention_multi off the matrix pipe: a RoPE / append launch + simple_attn_kernel<T>
};

// the refusals of srgpt_decode_attention, in the order they win where a call hits several
enum AttnStatus {
  ATTN_OK,
  ATTN_MAX_POS_TOO_LONG,  // the VALU kernel's score buffer (ATTN_DEC_CHUNK_MAX keys per split, ATTN_DEC_SPLIT_MAX splits)
  ATTN_BAD_HEAD_DIM,      // not 16 / 32 / 64 / 128
  ATTN_BAD_GROUP,         // heads / kv_heads not 1 / 2 / 4 / 8
  ATTN_TOO_MANY_COLUMNS,  // srgpt_decode_attention_multi on the matrix pipe: T * G query heads do not fit the 16 columns
};

struct AttnPrefillRoute {
  AttnFamily family;
  int hdp;  // ATTN_FLASH: the padded head width (template argument): 32 / 64 / 96 / 128
  int grid_x, grid_y, grid_z, block;
};

struct AttnDecodeRoute {
  AttnStatus status;
  AttnFamily family;
  int G;       // query heads per kv head (template argument)
  int nsplit;  // blocks per (sequence, kv head)
  int kpb;     // ATTN_DECODE_MFMA: keys per block (a multiple of 64); ATTN_DECODE_VALU: 0, the chunk follows the sequence length
  int n_attn;  // attention blocks of the launch (prefetch blocks come behind them); 256 threads each
};

constexpr int ATTN_FLASH_QBLK = 64;  // query rows per block of the flash kernel
// byte offsets inside a (batch, head) K / V slice are 32-bit in the flash kernel (buffer descriptors)
constexpr int64_t ATTN_FLASH_SLICE_SPAN_LIMIT = (int64_t)1 << 31;
constexpr int ATTN_DEC_CHUNK_MAX = 256;  // keys per split whose scores the VALU kernel holds in LDS
constexpr int ATTN_DEC_SPLIT_MAX = 64;   // splits per (sequence, kv head): one lane of the merging wave each
constexpr int ATTN_DEC_MFMA_KEYS = 64;   // keys per MFMA block and step: 4 waves x 16

// ------------------------------------------------------------------------------------------------
// The decode workspace (include/srgpt.h, srgpt_decode_attn_ws_floats): B * Hq * ATTN_DEC_SPLIT_MAX partial rows of D + 2 floats (the
// unnormalised output, then the split's maximum and sum), head-major -- the G heads of a (sequence, kv head) group are adjacent --
// and behind them the arrival tickets, one int per (sequence, kv head).  B * Hq ints are reserved and re-armed (the size the ABI
// has always reported: Hkv is not among its arguments); the kernels use the first B * Hkv <= B * Hq of them.
// ------------------------------------------------------------------------------------------------
constexpr size_t attn_ws_partial_floats(int B, int Hq, int D) { return (size_t)B * Hq * ATTN_DEC_SPLIT_MAX * (D + 2); }
constexpr size_t attn_ws_tickets_reserved(int B, int Hq) { return (size_t)B * Hq; }
constexpr size_t attn_ws_tickets_used(int B, int Hkv) { return (size_t)B * Hkv; }
constexpr size_t attn_ws_floats(int B, int Hq, int D) { return attn_ws_partial_floats(B, Hq, D) + attn_ws_tickets_reserved(B, Hq); }
// the partials of the G heads of (sequence b, kv head hk)
constexpr size_t attn_ws_group(int b, int hk, int Hkv, int G, int D) {
  return (((size_t)b * Hkv + hk) * G) * (size_t)ATTN_DEC_SPLIT_MAX * (D + 2);
}
// inside a group: the row of (head gq of the group, split)
constexpr size_t attn_ws_row(int gq, int split, int D) { return ((size_t)gq * ATTN_DEC_SPLIT_MAX + split) * (D + 2); }
// the group's ticket among the ints behind the partials (`tickets` = the workspace + attn_ws_partial_floats)
template <typename P>
constexpr P* attn_ws_ticket(P* tickets, int b, int hk, int Hkv) { return tickets + (size_t)b * Hkv + hk; }

namespace attn_route_detail {

constexpr int ceil_div(int a, int b) { return (a + b - 1) / b; }

// bf16, head_dim 128 (every LLM geometry) and a group the B operand's 16 columns hold
constexpr bool decode_use_mfma(bool bf16, int D, int G) { return bf16 && D == 128 && (G == 1 || G == 2 || G == 4 || G == 8); }

// the MFMA kernel: a block owns a FIXED range of 64 keys (4 waves x 16), so ceil(capacity / 64) blocks per (sequence, kv head) --
// those past the sequence end leave at once and the merge skips them; beyond 64 splits the ranges grow in steps of 64 keys and the
// waves loop
constexpr int decode_nsplit_mfma(int max_pos) {
  int n = ceil_div(max_pos, ATTN_DEC_MFMA_KEYS);
  if (n < 1) n = 1;
  if (n > ATTN_DEC_SPLIT_MAX) n = ATTN_DEC_SPLIT_MAX;
  return n;
}

// the VALU kernel, splits per (sequence, kv head): enough blocks for ~2 per CU, capped at 16 for a single sequence (it needs them to
// spread its K/V rows over the chip) and at 8 from two sequences up (the batch already spreads; more splits only multiply the merge
// work -- decode step at 4 sequences 3.44 ms with 8 splits vs 3.47 with 16, at 8 sequences 3.60 / 3.66,
// profiles/r02_decode_splits.txt), never fewer than the score buffer requires (ATTN_DEC_CHUNK_MAX keys per split)
constexpr int decode_nsplit_valu(int max_pos, int B, int Hkv, int cus) {
  int want = ceil_div(2 * cus, Hkv * B);
  const int cap = B == 1 ? 16 : 8;
  if (want > cap) want = cap;
  if (want < 1) want = 1;
  int n = ceil_div(max_pos, ATTN_DEC_CHUNK_MAX);
  if (n < want) n = want;
  if (n > ATTN_DEC_SPLIT_MAX) n = ATTN_DEC_SPLIT_MAX;
  return n;
}

}  // namespace attn_route_detail

// srgpt_attention (prefill / ViT) for validated arguments: strides in elements, q/k/v 16-byte and o 8-byte aligned?, scale > 0?
// The MFMA kernel loads 16-byte slots (head_dim and every stride a multiple of 8, head_dim <= 128), takes the row maximum before
// scaling (scale > 0) and addresses a (batch, head) slice with 32-bit byte offsets; anything else goes to the one-wave-per-row kernel.
// srgpt_attention_append (a per-row query position instead of the uniform offset Tk - Tq) takes this route UNCHANGED, evaluated with
// Tk = the caller's bound on the keys any row may see: no row reads past min(kv_len[b], Tk), so the span test covers it, and the grid
// depends on Tq alone.
inline AttnPrefillRoute attn_prefill_route(bool bf16, int D, int Tq, int Tk, int Hq, int B, int64_t q_bs, int64_t q_ts, int64_t q_hs,
                                           int64_t k_bs, int64_t k_ts, int64_t k_hs, int64_t v_bs, int64_t v_ts, int64_t v_hs,
                                           bool qkv_aligned16, bool o_aligned8, bool scale_positive) {
  const bool vec_ok = D % 8 == 0 && D <= 128 && q_ts % 8 == 0 && q_hs % 8 == 0 && q_bs % 8 == 0 && k_ts % 8 == 0 && k_hs % 8 == 0 &&
                      k_bs % 8 == 0 && v_ts % 8 == 0 && v_hs % 8 == 0 && v_bs % 8 == 0 && qkv_aligned16 && o_aligned8;
  // bytes of a slice the kernel may address: Tk rows and four key tiles of 64 beyond them, on the wider of the two row strides
  const int64_t span = ((int64_t)Tk + 4 * 64) * (k_ts > v_ts ? k_ts : v_ts) * 2;
  if (bf16 && vec_ok && scale_positive && span < ATTN_FLASH_SLICE_SPAN_LIMIT)
    return AttnPrefillRoute{ATTN_FLASH, (D + 31) / 32 * 32, attn_route_detail::ceil_div(Tq, ATTN_FLASH_QBLK), Hq, B, 256};
  return AttnPrefillRoute{ATTN_ONE_WAVE, 0, Tq, Hq, B, 64};
}

// srgpt_decode_attention for validated arguments (Hq % Hkv == 0): one new token per sequence against a cache of max_pos positions
inline AttnDecodeRoute attn_decode_route(bool bf16, int B, int Hq, int Hkv, int D, int max_pos, int cus) {
  using namespace attn_route_detail;
  AttnDecodeRoute r{ATTN_OK, ATTN_DECODE_VALU, Hq / Hkv, 0, 0, 0};
  if (decode_use_mfma(bf16, D, r.G)) {
    r.family = ATTN_DECODE_MFMA;
    r.nsplit = decode_nsplit_mfma(max_pos);
    r.kpb = ceil_div(ceil_div(max_pos, r.nsplit), ATTN_DEC_MFMA_KEYS) * ATTN_DEC_MFMA_KEYS;  // 64 keys up to 64 x 64 cached positions
  } else {
    r.nsplit = decode_nsplit_valu(max_pos, B, Hkv, cus);
  }
  r.n_attn = Hkv * r.nsplit * B;
  // VALU kernel: a split's scores live in LDS (sc[G][ATTN_DEC_CHUNK_MAX]): the longest chunk is ceil(max_pos / nsplit) keys
  if (r.family == ATTN_DECODE_VALU && ceil_div(max_pos, r.nsplit) > ATTN_DEC_CHUNK_MAX) r.status = ATTN_MAX_POS_TOO_LONG;
  else if (D != 16 && D != 32 && D != 64 && D != 128) r.status = ATTN_BAD_HEAD_DIM;
  else if (r.G != 1 && r.G != 2 && r.G != 4 && r.G != 8) r.status = ATTN_BAD_GROUP;
  return r;
}

// ------------------------------------------------------------------------------------------------
// srgpt_decode_attention_multi: T new tokens per sequence (the next token and T - 1 drafted ones) against the cache in ONE launch.
// The MFMA kernel puts query head g of token t into column c = t * G + g of the B operand, so T * G <= ATTN_DEC_MULTI_COLS; key
// ranges, splits and keys per block are attn_decode_route's (they depend on max_pos alone).  The workspace is the decode workspace
// with T * Hq "heads": the T * G columns of a (sequence, kv head) group are adjacent (attn_ws_group with G = cols, attn_ws_row with
// gq = the column), the tickets -- B * Hq reserved, B * Hkv used -- lie behind the B * T * Hq * ATTN_DEC_SPLIT_MAX partial rows.
// Everything off the matrix pipe (fp32, other head widths: the parity path) is a composition of existing launches and uses no
// workspace: nsplit = kpb = blocks = 0.
// ------------------------------------------------------------------------------------------------
constexpr int ATTN_DEC_MULTI_COLS = 16;  // columns of the MFMA B operand

struct AttnDecodeMultiRoute {
  AttnStatus status;  // ATTN_OK or ATTN_TOO_MANY_COLUMNS
  AttnFamily family;  // ATTN_DECODE_MULTI_MFMA / ATTN_DECODE_MULTI_COMPOSED
  int G, T;
  int cols;    // T * G: live columns of the B operand (ATTN_DECODE_MULTI_MFMA)
  int nc;      // ... rounded up to 2 / 4 / 8 / 16: the kernel's template argument (0: no MFMA instance)
  int nsplit;  // blocks per (sequence, kv head)
  int kpb;     // keys per block
  int blocks;  // blocks of the launch, 256 threads each
  size_t ws_floats;  // srgpt_decode_attn_multi_ws_floats(B, T, Hq, D)
};

constexpr size_t attn_multi_ws_partial_floats(int B, int T, int Hq, int D) { return attn_ws_partial_floats(B, T * Hq, D); }
constexpr size_t attn_multi_ws_floats(int B, int T, int Hq, int D) {
  return attn_multi_ws_partial_floats(B, T, Hq, D) + attn_ws_tickets_reserved(B, Hq);
}
// the most tokens per sequence the MFMA kernel takes at a group size (0: the group is not one of its instances)
constexpr int attn_decode_multi_cap(int G) { return (G == 1 || G == 2 || G == 4 || G == 8) ? ATTN_DEC_MULTI_COLS / G : 0; }

// srgpt_decode_attention_multi for validated arguments (T >= 1, Hq % Hkv == 0)
inline AttnDecodeMultiRoute attn_decode_multi_route(bool bf16, int B, int T, int Hq, int Hkv, int D, int max_pos) {
  using namespace attn_route_detail;
  AttnDecodeMultiRoute r{ATTN_OK, ATTN_DECODE_MULTI_COMPOSED, Hq / Hkv, T, T * (Hq / Hkv), 0, 0, 0, 0, attn_multi_ws_floats(B, T, Hq, D)};
  if (!decode_use_mfma(bf16, D, r.G)) return r;
  r.family = ATTN_DECODE_MULTI_MFMA;
  r.nsplit = decode_nsplit_mfma(max_pos);
  r.kpb = ceil_div(ceil_div(max_pos, r.nsplit), ATTN_DEC_MFMA_KEYS) * ATTN_DEC_MFMA_KEYS;  // attn_decode_route's ranges
  r.blocks = Hkv * r.nsplit * B;
  if (r.cols > ATTN_DEC_MULTI_COLS) r.status = ATTN_TOO_MANY_COLUMNS;
  else r.nc = r.cols <= 2 ? 2 : r.cols <= 4 ? 4 : r.cols <= 8 ? 8 : 16;
  return r;
}
