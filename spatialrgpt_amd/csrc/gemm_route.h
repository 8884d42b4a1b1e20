// Which kernel a GEMM runs on, and how K is split: the host-side selection of gemm.hip / gemm_f8.hip as pure functions of the
// shape, the CU count and the split-K workspace.  Plain C++ (no HIP): tests/test_host_gemm_route.py compiles this header alone and
// pins the route of every workload shape (tests/golden/gemm_routes.json) -- every threshold below was calibrated on the MI355X,
// and all routes compute the same bits, so nothing else notices a slipped comparison.
#pragma once
#include <stdint.h>

enum GemmFamily {
  GEMM_F32_SIMPLE,   // gemm_f32_simple (gemm.hip): the fp32 parity path, 64 x 64 tiles
  GEMM_WHOLE_M_288,  // gemm_bf16_288_kernel (gemm288.hip): one tile of up to 272 rows in M, 128 columns
  GEMM_TILE_256,     // gemm_bf16_256_kernel (gemm256.hip; gemm_f8_256_kernel for fp8 x fp8): 256 x 256 tiles
  GEMM_GLDS,         // gemm_bf16_glds<bm, 128, nbuf> (gemm.hip): 128 / 96 / 64 x 128 tiles, direct-to-LDS staging
};

struct GemmRoute {
  GemmFamily family;
  int bm;               // rows of a tile
  int nbuf;             // LDS stage buffers (GEMM_GLDS: the kernel's template argument)
  int splits;           // K splits (1: none); > 1 needs splits * M * N * 4 bytes of workspace and a slab reduction
  int tiles_per_split;  // K tiles per split; splits * tiles_per_split >= K tiles and no split is empty
};

namespace gemm_route_detail {

inline long cdivl(long a, long b) { return (a + b - 1) / b; }

// `sp` splits wanted over `nk` K tiles -> the route's split fields, without an empty last split
inline GemmRoute with_split(GemmFamily family, int bm, int nbuf, int nk, int sp) {
  GemmRoute r{family, bm, nbuf, 1, nk};
  if (sp > 1) {
    r.tiles_per_split = (int)cdivl(nk, sp);
    r.splits = (int)cdivl(nk, r.tiles_per_split);  // no empty split
  }
  return r;
}

// K splits of a grid of `tiles` 256 x 256 tiles that leaves CUs idle: `want` splits would fill the chip; at most 4, at least
// `min_tiles` K tiles each, the fp32 slabs inside the workspace (deterministic slabs, reduced in slab order)
inline int split_256(long tiles, int cus, long want, int nk, int min_tiles, int64_t slab_bytes, bool have_ws, int64_t ws_bytes) {
  if (tiles >= cus || !have_ws) return 1;
  int sp = (int)want;
  if (sp < 1) sp = 1;
  if (sp > 4) sp = 4;
  while (sp > 1 && (nk / sp < min_tiles || sp * slab_bytes > ws_bytes)) --sp;
  return sp;
}

}  // namespace gemm_route_detail

// srgpt_gemm on fp32 operands: one kernel, no split
inline GemmRoute gemm_route_f32() { return GemmRoute{GEMM_F32_SIMPLE, 64, 1, 1, 0}; }

// srgpt_gemm / srgpt_gemm_norm / srgpt_gemm_rope_kv_append on bf16 operands: C[M, N] = A[M, K] W[N, K]^T on `cus` compute units,
// `ws_bytes` of split-K workspace when `have_ws`
inline GemmRoute gemm_route(int M, int N, int K, int cus, bool have_ws, int64_t ws_bytes) {
  using namespace gemm_route_detail;
  const int64_t slab_bytes = (int64_t)M * N * 4;
  // ---- 288 x 128 whole-M kernel (gemm288.hip) for the bs = 1 prefill products (224 < M <= 272): W crosses the global -> LDS path
  //      once, requests three K tiles deep.  Column tiles x K splits should come to about one block per CU.
  {
    const int nk = K / 64;
    const int gx = (int)cdivl(N, 128);
    // measured at M = 259 (profiles/r04_gemm288.txt): gate/up 106.5 -> 84.2 us, down 64.8 -> 50.6, q/k/v 33.8 -> 32.0; o (27.5 vs
    // 27.9: 8 K tiles per block once K is split for 256 CUs, three of them pipeline fill) stays on the small tiles
    bool use288 = K % 64 == 0 && nk >= 4 && M > 224 && M <= 272 && (int64_t)N * K >= (int64_t)24 << 20;
    int sp = 1;
    if (use288) {  // one 272-row tile in M: the grid is gx column tiles x sp K splits
      if (gx < cus * 3 / 4 && have_ws) {
        sp = (cus + gx / 2) / gx;
        if (sp > nk / 8) sp = nk / 8;  // keep >= 8 K tiles per split: three of them are pipeline fill
        if (sp > 8) sp = 8;
        while (sp > 1 && sp * slab_bytes > ws_bytes) --sp;
        if (sp < 1) sp = 1;
      }
      if ((long)gx * sp < cus / 2) use288 = false;  // too few blocks to fill the chip: the small tiles overlap better
    }
    if (use288) return with_split(GEMM_WHOLE_M_288, 272, 3, nk, sp);
  }
  // ---- 256 x 256 eight-wave kernel (gemm256.hip); rule calibrated on MI355X measurements (profiles/r02_gemm256_*.txt,
  //      profiles/r02_gemm_final.txt: one block per CU, ~15 us of launch + prologue + epilogue per round of tiles) ----
  //   K >= 2048: it wins or ties on every shape with M >= 384 (prefill b8 qkv 111 vs 172 us, down 334 vs 455, b4 down 140 vs 212);
  //              an under-filled grid splits K (deterministic slabs) up to ~1.1 rounds of blocks
  //   K <  2048: the fixed cost per round is a quarter of the tile time, so only when the last round is nearly full
  //              (>= 88 %: ViT out-proj 50 vs 62 us; ViT qkv / fc1 at 84 / 76 % stay on the small-tile kernel: 131 vs 143 us)
  {
    const int nk = K / 64;
    const long t256 = cdivl(M, 256) * cdivl(N, 256);
    // M >= 384 and at most 25 % of padded rows (M = 518 would fill 3 row tiles to 67 %)
    bool use256 = K % 64 == 0 && K >= 256 && M >= 384 && (long)M * 4 >= cdivl(M, 256) * 256 * 3;
    int sp = 1;
    if (use256) {
      if (K >= 2048) {
        sp = split_256(t256, cus, (cus * 11 / 10 + t256 / 2) / t256, nk, 8, slab_bytes, have_ws, ws_bytes);
      } else {
        const long rounds = (t256 + cus - 1) / cus;
        use256 = t256 * 100 >= rounds * cus * 88;
      }
    }
    if (use256) return with_split(GEMM_TILE_256, 256, 2, nk, sp);
  }
  // ---- direct-to-LDS kernel: tile / split-K selection, fill the 256 CUs with >= ~2 blocks each ----
  const long t128 = cdivl(M, 128) * cdivl(N, 128);
  const long t64x128 = cdivl(M, 64) * cdivl(N, 128);
  const int nk = (int)cdivl(K, 64);
  const bool pad_waste = cdivl(M, 128) * 128 * 10 > cdivl(M, 64) * 64 * 11;  // > 10 % fewer padded rows with BM = 64
  // 128x128 only when it alone fills the chip at 4 blocks per CU; below that 64x128 has twice the blocks to overlap
  // (measured with the direct-to-LDS kernel: M=1458 N=4304 K=1152: 32.5 us vs 46.1 us; equal at 4096^3)
  if (!(t128 < 1024 || pad_waste)) return with_split(GEMM_GLDS, 128, 1, nk, 1);
  int bm = 64, splits = 1;
  // 96-row tiles (three 32-row MFMA tiles per wave, 1 x 4 waves) where they do not pad M by more than 8 % over 64-row tiles:
  // this kernel is bound by the global -> LDS fill rate, and a 96x128 step moves 17.8 B/kFLOP against 23.4 (M = 259 pads to
  // 288 instead of 320: gate/up 156 -> 106 us, ViT fc1 38 -> 25 us, profiles/r02_gemm_bm96.txt).  The split count keeps
  // following the 64-row tile count (the measured configuration).  (96x256 tiles measured: slower on every shape)
  if (M > 64 && cdivl(M, 96) * 96 * 100 <= cdivl(M, 64) * 64 * 108) bm = 96;
  if (t64x128 < 384 && have_ws) {
    splits = (int)((512 + t64x128 - 1) / t64x128);
    if (splits > nk / 8) splits = nk / 8;  // keep >= 8 K-tiles (512 columns of K) per split
    if (splits > 8) splits = 8;
    while (splits > 1 && splits * slab_bytes > ws_bytes) --splits;
    if (splits < 1) splits = 1;
  }
  GemmRoute r = with_split(GEMM_GLDS, bm, 1, nk, splits);
  if (bm == 96) {
    const long blocks = cdivl(N, 128) * cdivl(M, 96) * r.splits;
    // single buffer (5 blocks per CU overlap each other's K steps) only for un-split grids of >= 2 blocks per CU (gate/up 672,
    // ViT fc1 544 blocks: 106 vs 134 us, 25 vs 33 us); split-K and smaller grids double-buffer (q/k/v 34 vs 38 us)
    r.nbuf = r.splits <= 1 && blocks >= 2L * cus ? 1 : 2;
  } else {
    r.nbuf = t64x128 * r.splits < 3L * cus ? 2 : 1;
  }
  return r;
}

// srgpt_gemm_w8 (bf16 x fp8 weights, gemm256.hip<W8>) and srgpt_gemm_w8a8 (fp8 x fp8, gemm_f8.hip): always 256 x 256 tiles; K
// splits when the tiles do not fill the chip, whole splits per CU.  `nk` K tiles (of 64 / 128 elements), at least `min_tiles` of
// them per split: 8 for gemm256.hip, 4 for the fp8 x fp8 kernel, whose tile holds twice the K.
inline GemmRoute gemm_route_fp8(int M, int N, int nk, int min_tiles, int cus, bool have_ws, int64_t ws_bytes) {
  using namespace gemm_route_detail;
  const long tiles = cdivl(M, 256) * cdivl(N, 256);
  return with_split(GEMM_TILE_256, 256, 2, nk, split_256(tiles, cus, cus / tiles, nk, min_tiles, (int64_t)M * N * 4, have_ws, ws_bytes));
}

// srgpt_gemm_swiglu: does the whole-M kernel multiply gate and up columns in one block and apply the activation in its epilogue
// (225 .. 272 rows: the bs = 1 prefill; at least half a block per CU)?  Otherwise srgpt_gemm into the scratch + srgpt_silu_mul.
inline bool gemm_swiglu_fused_shape(int M, int I, int K, int cus) {
  return M > 224 && M <= 272 && K % 64 == 0 && K / 64 >= 4 && I % 64 == 0 && I / 64 >= cus / 2;
}

// srgpt_gemm_w4 / _norm / _rope_kv_append (MXFP4 codes as the weight operand): the route is gemm_route's, unchanged.  Does the kernel
// of route `r` multiply the codes itself?  Only the direct-to-LDS family has a W4 mode, and its code tile holds whole K tiles of 64;
// every other product expands the codes into the bf16 scratch first and runs the bf16 launch.
inline bool gemm_w4_in_kernel(const GemmRoute& r, int K) { return r.family == GEMM_GLDS && K % 64 == 0; }

// srgpt_gemm_w4_swiglu: the fused form runs on the whole-M kernel, which has no W4 mode; every other shape is the plain product of
// the stacked matrix [2 I, K]
inline bool gemm_swiglu_w4_in_kernel(int M, int I, int K, int cus, bool have_ws, int64_t ws_bytes) {
  return !gemm_swiglu_fused_shape(M, I, K, cus) && gemm_w4_in_kernel(gemm_route(M, 2 * I, K, cus, have_ws, ws_bytes), K);
}

// ---- the opt-in `_direct` forms of the four W4 entry points (srgpt_gemm_w4_direct ...): the whole-M kernel multiplies the codes too ----
// LDS of gemm_bf16_288_kernel's W4 instance (gemm288.hip): three stages of A 272 x 64 bf16 + W 128 x 32 B of codes, and behind them the
// E8M0 bytes of the block's 128 W rows over the block's own K tiles, [tile][row] as 16-bit pairs, a tile 4 bytes past 256 so that the
// staging writes of consecutive tiles fall into different banks.  The table has to fit what the stages leave of a CU's 160 KiB.
constexpr int GEMM288_LDS_MAX = 160 * 1024;
constexpr int GEMM288_W4_STAGES = 3 * (272 * 64 * 2 + 128 * 32);  // 114 KiB
constexpr int GEMM288_W4_SCALE_TILE = 128 * 2 + 4;                // bytes of the table per K tile
// the fit rule, shared by the route below and the kernel's launcher: `tiles` K tiles in a block's range
inline bool gemm288_w4_scales_fit(int tiles) {
  return tiles > 0 && (int64_t)tiles * GEMM288_W4_SCALE_TILE <= GEMM288_LDS_MAX - GEMM288_W4_STAGES;
}

// srgpt_gemm_w4_direct / _norm_direct / _rope_kv_append_direct: does the kernel of route `r` multiply the codes itself?  Wherever
// gemm_w4_in_kernel says so, and on the whole-M family (whose requirements K % 64 == 0 and >= 4 K tiles gemm_route has checked; they
// are repeated here because the kernel's W4 mode depends on them) when the scale bytes of a block's K range fit the LDS left over.
// The 256 x 256 tiles and K % 64 == 32 still expand.
inline bool gemm_w4_direct_in_kernel(const GemmRoute& r, int K) {
  if (gemm_w4_in_kernel(r, K)) return true;
  return r.family == GEMM_WHOLE_M_288 && K % 64 == 0 && K / 64 >= 4 && gemm288_w4_scales_fit(r.tiles_per_split);
}

// srgpt_gemm_w4_swiglu_direct: the fused whole-M shape (never split: a block's range is all of K) under the same conditions; every
// other shape is the plain product of the stacked matrix [2 I, K]
inline bool gemm_swiglu_w4_direct_in_kernel(int M, int I, int K, int cus, bool have_ws, int64_t ws_bytes) {
  if (gemm_swiglu_fused_shape(M, I, K, cus)) return gemm288_w4_scales_fit(K / 64);  // (the shape has K % 64 == 0 and >= 4 tiles)
  return gemm_w4_direct_in_kernel(gemm_route(M, 2 * I, K, cus, have_ws, ws_bytes), K);
}
