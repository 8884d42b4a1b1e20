// Which kernel a decode product runs on, with which template arguments and launch shape, and how a call of many rows is cut into
// weight passes: the host-side selection of gemv.hip / gemv_w8.hip / skinny.hip as pure functions of the shape and the CU count.
// Plain C++ (no HIP): tests/test_host_gemv_route.py compiles this header alone and pins the launch of every product of the decode
// step (tests/golden/gemv_routes.json) -- every threshold below was calibrated on the MI355X, and all routes compute the same bits,
// so nothing else notices a slipped comparison.
#pragma once
#include "pack13.h"  // the packed format's group size, for gemv_p13_launch

enum GemvFamily {
  GEMV_LDS,     // gemv_kernel<T, B, SWIGLU, NX, UB> (gemv.hip): VALU, 1 - 4 rows staged in LDS
  GEMV_REG,     // gemv_reg_kernel<SWIGLU, false, NIT> (gemv.hip): VALU, one bf16 row held in registers
  GEMV_W8,      // gemv_w8_kernel<1, SWIGLU, NX> (gemv_w8.hip): VALU, one bf16 row, fp8 weights
  GEMV_SKINNY,  // skinny_kernel<SWIGLU, NI, NW, W8, PUB, PK> (skinny.hip): MFMA, up to 16 bf16 rows
  GEMV_W4,      // gemv_w4_kernel<B, SWIGLU, NX> (gemv_w4.hip): VALU, 1 - 4 bf16 rows, MXFP4 weights (its own route functions below)
  GEMV_P13,     // gemv_p13_kernel<SWIGLU, NX> (gemv_p13.hip): VALU, one bf16 row, 13-bit packed bf16 weights (route functions below)
  GEMV_W4_MFMA, // skinny_kernel<SWIGLU, NI, NW, false, PUB, true, W4 = true> (skinny.hip): MFMA, up to 16 bf16 rows, packed MXFP4 weights
};

// How a call is cut: ceil(rows / chunk) launches of up to `chunk` rows, each streaming the weights once, ALL on `family` -- a
// single-row tail of a longer call (17, 33 rows) stays on the kernel its other rows took
struct GemvRoute {
  GemvFamily family;
  int chunk;
};

// VALU families (256 threads per block)
struct GemvValuLaunch {
  int B;          // rows (GEMV_LDS: the template argument)
  int NX;         // activation chunks a thread of the prologue holds in registers (GEMV_LDS, GEMV_W8)
  int UB;         // weight loads per batch (GEMV_LDS)
  int NIT;        // 64-lane chunk iterations per row (GEMV_REG: the template argument)
  int grid;
  long long lds;  // dynamic LDS bytes: the activation rows (GEMV_REG: none); above GEMV_LDS_CAP the launch is refused
  bool raise_lds_limit;  // more than the 48 KiB a kernel gets unasked: needs the GEMV_LDS_CAP attribute
};

// MFMA family (64 * NW threads per block)
struct GemvSkinnyLaunch {
  int NI;         // x rows staged per wave / 2
  int NW;         // waves per block (the K split)
  bool PUB, PK;   // statistics read from the producer's table; weights in the packed layout
  int grid, cw;   // block b owns output columns [b cw, (b + 1) cw)
  int gr_shift;   // log2 of the packed granule's rows (row-major: unused)
  int lds;        // dynamic LDS bytes (above 48 KiB the launcher raises the kernel's limit to exactly this)
};

// bf16 rows >= this go to the MFMA kernel of skinny.hip
constexpr int SKINNY_MIN_BATCH = 2;  // measured (round 3, profiles/r03_skinny_min_batch.txt): VALU wins at 1 row, MFMA from 2
// fp8 rows at or below this count take the one-row VALU kernel of gemv_w8.hip (which neither reads nor publishes row statistics)
constexpr int W8_VALU_MAX_BATCH = 1;  // 2 rows: the MFMA kernel is 7 % faster per step (round 3)
constexpr int GEMV_LDS_CAP = 150 * 1024;  // dynamic LDS a VALU kernel may ask for
constexpr int GEMV_ROWSS_SLOTS = 512;     // SRGPT_ROWSS_STRIDE (include/srgpt.h): one slot per producer block

namespace gemv_route_detail {

inline int ceil_div(int a, int b) { return (a + b - 1) / b; }

// 2+ bf16 rows on the MFMA kernel?  (the VALU kernels hold at most 4 rows)
inline bool rows_take_mfma(int rows, bool fp8) { return fp8 ? rows > W8_VALU_MAX_BATCH : rows > 4 || rows >= SKINNY_MIN_BATCH; }

// the register kernel's instances: K = 2560, 4096, 6912; longer rows (K = 11008, 14336: 88 - 112 VGPRs of activations, spills when
// unrolled) stay on the LDS kernel
inline bool reg_kernel_nit(int nit) { return nit == 5 || nit == 8 || nit == 14; }

// The grid of the VALU kernels, a wave per unit and four waves per block: two blocks per CU, one where the rows fill over 70 KiB of
// LDS.  (round 5, measured and not kept: 3 / 4 / 5 blocks per CU for the short launches -- q/k/v, o_proj, where a wave owns only
// 2 - 3 rows, i.e. 2 - 3 dependent memory round trips: 2.970 -> 2.998 / 3.009 / 3.017 ms per token; for all launches 3.037 / 3.049:
// profiles/r05_decode_step_ab.txt)
inline int valu_grid(int units, long long lds, int cus) {
  const int per_cu = lds > 70 * 1024 ? 1 : 2;
  int grid = ceil_div(units, 4);
  if (grid > cus * per_cu) grid = cus * per_cu;
  return grid < 1 ? 1 : grid;
}

// NXMAX of the VALU prologues: 2 chunks of 16 activation bytes per thread cover 512, else 8 (past 2048 the kernel loops)
inline int valu_nx(int chunks) { return chunks <= 512 ? 2 : 8; }

}  // namespace gemv_route_detail

// srgpt_gemv (bf16 / fp32), srgpt_gemv_w8 (fp8) and srgpt_gemv_rowss (bf16 or fp8, with the statistics hand-off): `rows` x K
// activations, bf16 or fp32 (the parity dtype of the tiny models); fp8: OCP e4m3 weights, bf16 activations; norm: RMSNorm prologue
inline GemvRoute gemv_route(int rows, int K, bool bf16, bool fp8, bool norm) {
  using namespace gemv_route_detail;
  if (fp8) {
    // one row: VALU kernel, like the bf16 path (its 16-byte weight chunks need K % 16 == 0); else 16 rows per weight pass
    if (!rows_take_mfma(rows, true) && K % 16 == 0) return GemvRoute{GEMV_W8, rows};
    return GemvRoute{GEMV_SKINNY, 16};
  }
  if (bf16) {
    if (rows_take_mfma(rows, false)) return GemvRoute{GEMV_SKINNY, 16};  // 16 rows = the M side of one MFMA tile
    // measured (scripts/experiments/ubench_gemv_c.hip): without the fused RMSNorm the register variant saves 0.6-0.8 us per launch
    // (o_proj 8.5 -> 7.9 us); with it every wave normalises the whole row redundantly and loses ~1 us -> LDS kernel
    if (rows == 1 && !norm && reg_kernel_nit(ceil_div(K / 8, 64))) return GemvRoute{GEMV_REG, 1};
    return GemvRoute{GEMV_LDS, rows};
  }
  // fp32: up to 4 rows per launch; a longer call takes 4 at a time, fewer where 4 rows of K do not fit the LDS cap
  if (rows <= 4) return GemvRoute{GEMV_LDS, rows};
  int step = 4;
  while (step > 1 && (long long)step * K * 4 > GEMV_LDS_CAP) --step;
  return GemvRoute{GEMV_LDS, step};
}

// Does (rows, dtype, fp8) take the kernel with the row-statistics hand-off (srgpt_gemv_rowss)?  The MFMA kernel, and a table with
// one slot per producer block (two 4-wave blocks per CU).
inline bool gemv_rowss_supported(int rows, bool bf16, bool fp8, int cus) {
  return bf16 && rows >= 2 && 2 * cus <= GEMV_ROWSS_SLOTS && gemv_route_detail::rows_take_mfma(rows, fp8);
}

// one launch of a VALU family: B rows (one chunk of the route)
inline GemvValuLaunch gemv_valu_launch(GemvFamily family, int B, int N, int K, bool bf16, bool swiglu, int cus) {
  using namespace gemv_route_detail;
  const int vec = bf16 ? 8 : 4;  // activation elements per 16-byte chunk
  GemvValuLaunch l{B, 0, 8, 0, 0, (long long)B * K * (bf16 ? 2 : 4), false};
  l.raise_lds_limit = l.lds > 48 * 1024;
  l.NX = valu_nx(B * (K / vec));
  if (family == GEMV_W8) {  // a unit is two output columns
    l.grid = valu_grid((N + 1) / 2, l.lds, cus);
    return l;
  }
  l.grid = valu_grid(N, l.lds, cus);
  l.NIT = ceil_div(K / vec, 64);
  if (family == GEMV_REG) {
    l.lds = 0;
    l.raise_lds_limit = false;
    return l;
  }
  // batches of 7 loads for rows whose chunk iterations are a multiple of 7 and not of 8 (K = 14336, down_proj: 28 iterations are
  // 4 batches of 7, where batches of 8 spent every row's fourth batch half on clamped re-reads of the row's last chunk)
  if (!swiglu && B == 1 && bf16 && l.NIT % 7 == 0 && l.NIT % 8 != 0 && l.NX == 8) l.UB = 7;
  return l;
}

// dynamic LDS of a skinny_kernel block: per wave an activation stage of 2 NI rows and (row-major weights) a 16-row weight stage,
// rows padded to 544 bytes; reused for the cross-wave reduction of 4 sub-units x 64 lanes x 4 floats per wave
constexpr int GEMV_SKINNY_ROW_BYTES = 512 + 32, GEMV_SKINNY_SUBUNITS = 4;
constexpr int gemv_skinny_lds(int NI, int NW, bool PK) {
  const int stages = NW * (2 * NI + (PK ? 0 : 16)) * GEMV_SKINNY_ROW_BYTES, reduction = NW * GEMV_SKINNY_SUBUNITS * 64 * 4 * 4;
  return stages > reduction ? stages : reduction;
}

// one launch of the MFMA family: up to 16 rows (one chunk of the route)
inline GemvSkinnyLaunch gemv_skinny_launch(int rows, int N, bool norm, bool ss_in, int packed, int cus) {
  using namespace gemv_route_detail;
  GemvSkinnyLaunch l{};
  l.NI = rows <= 4 ? 2 : rows <= 8 ? 4 : 8;
  // Two 4-wave blocks per CU, or one 8-wave block per CU; both split the columns evenly over their blocks.  Measured per decode
  // step (profiles/r02_skinny_ab.txt): 4-wave blocks win (o_proj 8.8 vs 9.7 us, fp8 gate/up 27.4 vs 30.4) except where a block
  // would own few columns AND has the RMSNorm statistics to compute first (q/k/v: 24 columns per CU, 14.1 vs 14.3 us bf16,
  // 12.3 vs 13.7 fp8) -- there the prologue is shared by twice the threads.
  const int ncol = ceil_div(N, cus);  // output columns per CU
  l.NW = norm && ncol <= 32 ? 8 : 4;
  const int blocks = l.NW == 8 ? cus : 2 * cus;
  l.cw = ceil_div(N, blocks);
  if (l.cw < 16) l.cw = 16;  // at least one whole 16-column tile
  l.gr_shift = packed == 16 ? 4 : packed == 8 ? 3 : 2;
  if (packed) l.cw = ceil_div(l.cw, packed) * packed;  // whole granules
  l.grid = ceil_div(N, l.cw);
  l.PUB = ss_in;
  l.PK = packed != 0;
  l.lds = gemv_skinny_lds(l.NI, l.NW, l.PK);
  return l;
}

// ---- srgpt_gemv_w4 (gemv_w4.hip): MXFP4 weights, bf16 activations.  One kernel family for every row count: there is no MFMA kernel
// for the format, so a longer call is cut into launches of at most W4_MAX_ROWS rows (the kernel's template argument), each a pass
// over the code bytes.  A unit (one wave's work item) is W4_UNIT_COLS output columns.  A K = 4096 row of codes is only two 1-KiB
// wave loads, so four columns would put gemv_w8.hip's 8 (SwiGLU: 16) KiB per wave in flight -- measured, that is SLOWER than two
// (profiles/mxfp4.txt: the batch-1 step 1.48 ms at 2 columns, 1.64 at 4, 1.98 at 8; per product 2 wins or ties at 1 - 2 rows): twice
// the units give the short launches twice the waves, and 4 - 8 KiB per wave over 8 waves per CU already cover the HBM latency.
constexpr int W4_MAX_ROWS = 4;
constexpr int W4_UNIT_COLS = 2;

inline GemvRoute gemv_w4_route(int rows) { return GemvRoute{GEMV_W4, rows < W4_MAX_ROWS ? (rows < 1 ? 1 : rows) : W4_MAX_ROWS}; }

// one launch: B rows (one chunk of gemv_w4_route); K % 32 == 0
inline GemvValuLaunch gemv_w4_launch(int B, int N, int K, bool swiglu, int cus) {
  using namespace gemv_route_detail;
  (void)swiglu;  // a SwiGLU unit is the same W4_UNIT_COLS output columns (twice the weight rows)
  GemvValuLaunch l{B, 0, 0, 0, 0, (long long)B * K * 2, false};
  l.raise_lds_limit = l.lds > 48 * 1024;
  l.NX = valu_nx(B * (K / 8));
  l.NIT = ceil_div(K / 32, 64);
  l.grid = valu_grid(ceil_div(N, W4_UNIT_COLS), l.lds, cus);
  return l;
}

// ---- srgpt_gemv_w4p (gemv_w4p.hip -> skinny.hip) and the decode-shaped steps of an MXFP4 engine (model.hip): the MFMA product over
// the packed copy of a code array (srgpt_pack_mxfp4), where the step's matrices are bound (mxfp4_bind.h).  `bound`: every layer
// matrix of the engine has a packed copy of its shape.  Unbound, or below W4_MFMA_MIN_ROWS rows, the route is gemv_w4_route's; from
// the threshold on every pass is up to 16 rows on the MFMA kernel, launched as gemv_skinny_launch(rows, N, norm, ss_in,
// W4_GRANULE_ROWS, cus) says: the bf16 kernel's NI / NW rule, cw rounded to whole granules.
// W4_MFMA_MIN_ROWS = 2, measured per product at the 8B geometry on the MI355X (profiles/mxfp4_mfma.txt, us per launch, VALU kernel |
// MFMA product): 1 row q/k/v 6.1 | 8.3, o_proj 5.0 | 5.0, gate/up 13.6 | 15.0, down_proj 11.1 | 8.4; 2 rows 8.8 | 8.2, 6.9 | 5.0,
// 19.3 | 15.1, 14.4 | 8.5; 4 rows 12.6 | 8.3, 9.3 | 5.2, 28.1 | 15.3, 24.4 | 8.9; 16 rows 48.4 | 10.8, 35.7 | 5.8, 109.9 | 20.9, 96.2 | 13.0
// (the spread of a line's calls is under 3 %, between two processes under 1 %).  From 2 rows on the MFMA product wins EVERY product,
// so the threshold is one constant and the route takes no shape; at one row it wins down_proj alone and the step keeps the VALU kernel
// (whole steps: lookup K = 1 1.99 -> 1.53 ms, batch 8 5.27 -> 1.63).
constexpr int W4_MFMA_MIN_ROWS = 2;
constexpr int W4_GRANULE_ROWS = 16;  // SRGPT_MXFP4_GRANULE (include/srgpt.h): weight rows per granule of the packed array
constexpr int W4_CELL_K = 128;       // k per cell: one 16-byte load per lane = the B fragments of four MFMA k steps

inline GemvRoute gemv_w4_step_route(int rows, bool bound) {
  if (!bound || rows < W4_MFMA_MIN_ROWS) return gemv_w4_route(rows);
  return GemvRoute{GEMV_W4_MFMA, 16};
}

// ---- the wide pass (opt-in: srgpt_gemv_rowss_wide, srgpt_gemv_w4p_wide, srgpt_llm_weights::decode_pass_rows = 32): a chunk of 17 - 32
// rows on the NI = 16 instances of skinny_kernel, two 16-row M tiles against one stream of the weights.  pass_rows: 32 asks for it;
// anything else, or a call of 16 rows or fewer, is the route above for the same call (w4: the MFMA leg srgpt_gemv_w4p always takes).
// A call is cut into chunks of 32 and a tail; a tail of 16 rows or fewer takes the 16-row launch of its row count (40 = 32 + 8,
// 33 = 32 + 1).  This function is the one place that decides which products run wide.
constexpr int GEMV_WIDE_ROWS = 32;
// is there a wide instance of skinny_kernel for these weights?  (all but packed bf16: see gemv_wide_route)
constexpr bool gemv_wide_has_instance(bool fp8, int packed, bool w4) { return fp8 || w4 || packed == 0; }

inline GemvRoute gemv_wide_route(int rows, int K, bool fp8, int packed, bool w4, bool norm, bool swiglu, int pass_rows) {
  const GemvRoute base = w4 ? gemv_w4_step_route(W4_MFMA_MIN_ROWS, true) : gemv_route(rows, K, true, fp8, norm);
  if (pass_rows != GEMV_WIDE_ROWS || rows <= 16) return base;
  if (base.family != GEMV_SKINNY && base.family != GEMV_W4_MFMA) return base;
  (void)swiglu;
  // Measured on the MI355X at the 8B geometry (profiles/wide_decode.txt; us per launch at 17 / 32 rows, two 16-row passes -> wide; the
  // min .. max of a line's calls is under 0.6 us, lm_head under 10): EVERY product of the three engine formats beats its two passes by
  // more than that spread, so no measured entry keeps a product at 16 --
  //   bf16 row-major   q/k/v 24.7 -> 15.4 / 28.1 -> 16.0, o 17.2 -> 10.5 / 18.7 -> 11.1, gate/up 74.1 -> 41.4 / 75.2 -> 42.9,
  //                    down 43.3 -> 26.8 / 46.4 -> 29.3, lm_head 342.9 -> 180.2 / 360.8 -> 189.3
  //   fp8 packed       q/k/v 16.8 -> 13.8 / 19.0 -> 14.2, o 12.4 -> 8.9 / 13.7 -> 9.2, gate/up 45.7 -> 30.3 / 47.0 -> 31.7,
  //                    down 26.9 -> 22.5 / 31.6 -> 23.5, lm_head (fp8 row-major) 177.1 -> 124.9 / 200.8 -> 136.5
  //   MXFP4 packed     q/k/v 15.8 -> 13.4 / 18.6 -> 13.8, o 11.1 -> 8.7 / 12.1 -> 8.8, gate/up 31.4 -> 28.1 / 37.3 -> 28.9,
  //                    down 22.0 -> 21.4 / 26.4 -> 21.9 (the closest: 21.31 .. 21.58 against 21.84 .. 22.14 at 17 rows)
  // Products kept at passes of 16 rows, one line per entry with its reason (gemv_wide_has_instance is the launcher's side of it):
  // bf16 weights in the packed layout: skinny_kernel<false, 16, 8, false, true, true, false> spills 2 VGPRs (12 bytes of scratch), not built
  if (!gemv_wide_has_instance(fp8, packed, w4)) return base;
  return GemvRoute{base.family, GEMV_WIDE_ROWS};
}

// dynamic LDS of a wide block: stages of half a slice -- per wave 32 activation rows and (row-major weights) 16 weight rows of 128 k,
// padded to 288 bytes.  The reduction buffer holds both M tiles.
constexpr int GEMV_WIDE_ROW_BYTES = 256 + 32;
constexpr int gemv_wide_lds(int NW, bool PK) {
  const int stages = NW * (32 + (PK ? 0 : 16)) * GEMV_WIDE_ROW_BYTES, reduction = NW * 2 * GEMV_SKINNY_SUBUNITS * 64 * 4 * 4;
  return stages > reduction ? stages : reduction;
}

// one wide launch: 17 - 32 rows.  NW, cw, the grid and the granule are gemv_skinny_launch's for the same N and norm (they do not depend
// on the row count), so every row keeps the columns, the K range and the reduction order of its 16-row pass
inline GemvSkinnyLaunch gemv_wide_launch(int rows, int N, bool norm, bool ss_in, int packed, int cus) {
  GemvSkinnyLaunch l = gemv_skinny_launch(rows > 16 ? 16 : rows, N, norm, ss_in, packed, cus);
  l.NI = 16;
  l.lds = gemv_wide_lds(l.NW, l.PK);
  return l;
}

// bytes of the packed array of a [rows_total, K] code matrix (K % W4_CELL_K == 0): per granule and cell 64 code bytes and 4 scale
// bytes per row
inline long long gemv_w4p_packed_bytes(long long rows_total, int K) {
  const long long gran = (rows_total + W4_GRANULE_ROWS - 1) / W4_GRANULE_ROWS;
  return gran * (K / W4_CELL_K) * (68LL * W4_GRANULE_ROWS);
}

// ---- srgpt_gemv_p13 (gemv_p13.hip): bf16 weights in the lossless 13-bit code of pack13.h, one bf16 activation row.  The same
// unit / wave / grid decomposition as GEMV_LDS (a unit is one output row, or a gate and an up row), and the same bits.  A row is
// streamed in groups of 2048 weights = 4 wave loads (3328 bytes), and a batch is ONE group of each of the unit's rows (4 loads in
// flight per wave, SwiGLU 8).  Measured per product at one row on the MI355X (profiles/pack13.txt, us per launch, raw kernel first;
// g = groups per batch): lm_head 163.4 | g 1: 136.5, g 2: 138.8; gate/up 37.1 | g 1: 33.7, g 2: 34.3; q/k/v 10.3 | g 1: 11.8, g 2: 12.1;
// down_proj 21.1 | g 1: 26.6, g 7 (the whole row, 256 VGPRs): 30.3 -- the last two products stay on the raw kernels.
inline bool gemv_p13_eligible(int rows, int K) { return rows == 1 && p13_eligible(1, K); }
inline GemvRoute gemv_p13_route() { return GemvRoute{GEMV_P13, 1}; }  // one row per launch, and no call of more

// one launch: NIT = groups per row, UB = loads per batch and row, lds = the activation row padded to whole groups
inline GemvValuLaunch gemv_p13_launch(int N, int K, int cus) {
  using namespace gemv_route_detail;
  const int groups = p13_groups(K);
  GemvValuLaunch l{1, 0, 4, groups, 0, (long long)groups * P13_GROUP_WEIGHTS * 2, false};
  l.raise_lds_limit = l.lds > 48 * 1024;
  l.NX = valu_nx(K / 8);
  l.grid = valu_grid(N, l.lds, cus);
  return l;
}
