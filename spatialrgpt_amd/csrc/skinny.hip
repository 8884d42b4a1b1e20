// Batched decode-path weight-streaming product for 2..16 rows: out[b, n] = W[n, :] . x[b, :]   (bf16, HBM-bound)
//
// Same contract and fusions as the GEMV (gemv.hip: RMSNorm prologue, SwiGLU epilogue, residual add, fp32 logits), but
// above 4 rows the VALU formulation runs out of issue slots and LDS bandwidth (B LDS reads + 8 B FMAs per 16 weight
// bytes), so the 16-row batch becomes the M side of v_mfma_f32_16x16x32_bf16 and 16 weight rows the N side.
//
// Roofline: weight bytes read exactly once (non-temporal, each wave-instruction = 2 rows x 512 contiguous bytes).
// MFMA operand fragments need lane (r = l & 15, g = l >> 4) to hold 16 bytes of ROW r -- loading them straight from
// HBM puts 16 different rows in one instruction (64-byte pieces; measured slow, scripts/experiments/ubench_stream.hip), so each
// wave stages its 16 x 256 weight tile through a PRIVATE 8 KiB LDS region: 8 coalesced global loads -> 8 ds_write_b128
// -> 8 conflict-free ds_read_b128 fragments (row stride padded to 544 B).  The matching [rows][256] slice of the
// (normalised) activations goes through a second private region the same way (it comes from L2).  Nothing in the K loop
// is shared between waves, so there is NO block barrier in it (LDS ops of one wave execute in order) and the 8-12 waves
// of a CU drift apart like the GEMV's do: some stream while others multiply.
//
// Work decomposition: block b owns the `cw` consecutive output columns [b cw, (b + 1) cw), cut into tiles of 16 (the last one
// partial: its missing rows are not loaded); cw = ceil(N / blocks) makes every CU stream the same number of weight rows
// (6144 q/k/v columns = 24 per CU, 14336 gate/up pairs = 56 -- whole 16-column units left a quarter of the CUs with half the
// work).  A tile is one sub-unit (SwiGLU: the 16 gate rows + the 16 matching up rows = 2 sub-units); up to 4 sub-units per
// pass keep their 16x16 fp32 accumulators in registers (2 x 4 VGPRs each).  The waves of a block split K into one contiguous
// range of 256-wide slices each (round 3; interleaved slices before: see sl_of below), so every block uses all its
// waves even when it owns a single tile (o_proj / down_proj); their partial sums are added in a fixed order through LDS at the end
// of the pass (deterministic).
//
// The K loop is written for counted waits: every load in it is issued unconditionally, so the compiler can leave the
// prefetched stage in flight across the LDS writes (a branch around a load makes it wait for vmcnt(0) -- the prefetch was being
// drained every stage); the fragment reads of 4 k steps go out together in front of their MFMAs, which alternate between two
// accumulators (the compiler's own order was read -> wait -> MFMA per step: a full LDS latency each).
#include <stdlib.h>

#include <type_traits>

#include "common.h"
#include "gemv_route.h"
#include "internal.h"

namespace {

constexpr int WROWB = 512 + 32;        // bytes per staged weight row: 136 dwords = 8 mod 64 banks -> the lane groups of ds_read_b128
                                       // (MI355X guide, LDS table) hit distinct banks; 528 measured 30 % conflict cycles
constexpr int WSTAGEB = 16 * WROWB;    // weight stage per wave
constexpr int MAXSU = 4;               // sub-units (16-row weight tiles) accumulated per pass (8 for one 8-wave SwiGLU block per CU that
                                       // walks K once: measured equal, profiles/r06_skinny_gateup_8wave.txt)

constexpr int STAGE_DEPTH = 2;         // register ring depth of weight stages, bf16 and fp8 weights alike (an fp8 stage is half the
                                       // registers and half the bytes in flight; 3 / 4: profiles/r06_skinny_inflight.txt)
constexpr int FS_MAX = 4;              // MFMA k steps per fragment batch (8 LDS reads in flight per batch)

// NI = x rows staged per wave / 2: 2 (batch <= 4), 4 (batch <= 8) or 8 (batch <= 16).  NW = waves per block (the K split): two 4-wave
// blocks per CU, or one 8-wave block per CU (the launcher's rule, below).
// W8: the weights are OCP fp8 e4m3fn bytes with one fp32 scale per weight row (W8A16): a stage is 8 loads of 8 bytes per lane
// (2 rows x 256 bytes each), widened to bf16 (exact) on the way into LDS; the row scale multiplies the fp32 dot product.
// (Measured and dropped: 512-k fp8 slices with the raw bytes in LDS and the widening behind the fragment read -- a stage of as
// many bytes as a bf16 one -- 69.2 vs 63.7 us per layer at 8 rows: this kernel is not bound by bytes in flight.)
//
// Row statistics hand-off (round 5).  The RMSNorm in front of q/k/v, gate/up and lm_head needs sum(x^2) of every batch row; computed
// in the consumer, EVERY block re-read all rows (8 x 8 KiB at 8 rows) and reduced them through two block barriers before its first
// weight stage could even be requested: 7.7k of the q/k/v launch's 22k cycles at 8 fp8 rows (profiles/r02_skinny_stamps.txt).  The
// product that WRITES x (o_proj / down_proj with the residual add) has every element of it in a register: with `ss_out` it publishes,
// per block, the sum of squares of the columns it owns -- slot [row][block] of a [rows][SRGPT_ROWSS_STRIDE] fp32 table, slots past
// the grid zeroed, plain stores (the kernel boundary makes them visible).  A consumer instantiated with PUB reads its rows' 512 slots
// (one wave per row, two 16-byte loads per lane), adds them in a fixed order (lane-local, then the DPP / permlane tree) -- the
// result does not depend on which block finished first -- and goes straight to its weight stream: the statistics' loads, the first
// activation slice and the first weight stage are all requested back to back at kernel entry, one memory latency for the three.
// PK (round 6): the weights are read from the PACKED decode layout (srgpt_pack_decode_weights, include/srgpt.h): granules of `gr`
// rows (4 or 16) whose bytes are stored in MFMA-operand order -- [granule][k block][g = k / 8 % 4][row in granule][16 bytes] -- so
// that ONE coalesced 16-byte load per lane IS the B fragment of a k step (bf16: a k block = 32 k; fp8: 64 k = the fragments of two
// k steps); a wave-instruction reads 16 / gr pieces of gr x 64 contiguous bytes and a wave walks its K range through each granule
// sequentially.  The weights then never touch LDS: no ds_write / wave barrier / fragment ds_read per stage (the timing probe of
// round 5 priced them at 4 - 7 % of the fp8 layer, profiles/r05_skinny_probes.txt) and a block needs LDS only for its activation
// slices.  4-row granules keep every column split of the row-major kernel (24 q/k/v columns or 28 gate / up pairs per block);
// 16-row granules (1 KiB contiguous per instruction) stream the single-tile products faster (profiles/r06_skinny_packed_gr.txt).
// W4: the weights are MXFP4 codes in THEIR packed layout (srgpt_pack_mxfp4, include/srgpt.h; implies PK, excludes W8): a cell of a
// granule is 128 k = one 16-byte load per lane, dword s of which holds the lane's 8 codes of k step s, and a dword beside the codes
// holds the four E8M0 bytes of the lane's row.  A stage (256 k) is two such pairs -- an eighth of a bf16 stage's registers -- so the
// ring holds W4_DEPTH stages (3 with 8 staged rows, 2 with 16: the activation ring's registers are not there -- the deeper
// rings spilled 5 - 49 VGPRs in the o_proj / down_proj instances); a fragment is four v_cvt_scalef32_pk_bf16_fp4 (two codes each, the block scale `byte << 23` applied on
// the way: exact, code * 2^e has one mantissa bit) in front of the MFMA.  Everything that decides a bit -- NI / NW, the K range of a
// wave, the k of a step, the accumulator a step adds to, the reduction, the epilogues -- is the bf16 instance's: the same bits as
// that kernel over the dequantised matrix.
// WIDE (NI == 16, gemv_wide_launch of gemv_route.h): 17 - 32 rows in one weight pass, as TWO 16-row M tiles.  Every k step of a
// weight tile issues two v_mfma_f32_16x16x32_bf16 that share the weight fragment; each has its own activation fragment and its own
// accumulator (one per sub-unit and M tile, as in the NI == 8 instance).  NW, cw, the grid, a wave's K range, the k order, the
// wave-ordered reduction, the statistics and the epilogues are the NI == 8 instance's, so row r of a wide pass has the bits of a
// 16-row pass that holds it.  A slice of 32 activation rows is 64 registers per lane on its way into LDS, and beside a row-major weight
// stage the LDS for it is not there either (8 waves: 208 896 B), so a wide stage is HALF a slice: 128 k of 32 activation rows and of the
// 16 weight rows, staged rows padded to 288 B (72 dwords = 8 mod 64 banks, as 544 B).  A wave walks its 256-wide slices as pairs of such
// stages, in k order; a row-major wave load is then 4 rows x 256 bytes, a packed stage half the lane loads.
constexpr int W4_DEPTH = 4;
template <bool SWIGLU, int NI, int NW, bool W8, bool PUB, bool PK, bool W4>
__global__ __launch_bounds__(64 * NW, NW == 4 ? 2 : 1) void skinny_kernel(const bf16_t* __restrict__ x, const void* __restrict__ Wv,
                                                                          const float* __restrict__ wscale,
                                                                          const bf16_t* __restrict__ norm_w, float norm_eps,
                                                                          const bf16_t* __restrict__ residual, void* __restrict__ out,
                                                                          int B, int N, int K, int out_f32, int cw,
                                                                          const float* __restrict__ ss_in, float* __restrict__ ss_out,
                                                                          int gr_shift) {
  static_assert(!W4 || (PK && !W8), "MXFP4 weights are read from their packed layout only");
  constexpr int MT = NI == 16 ? 2 : 1;      // 16-row M tiles per pass
  constexpr int SK = MT == 2 ? 128 : 256;  // k per stage: a slice, or half of one (wide instances)
  constexpr int HS = 256 / SK;              // stages per slice
  // register ring depth of weight stages (half slices: half the bytes in flight -- deeper rings spilled 4 - 83 VGPRs in the wide instances)
  constexpr int DEPTH = !W4 || NI >= 8 ? STAGE_DEPTH : NI == 4 ? W4_DEPTH - 1 : W4_DEPTH;
  constexpr int XROWB = 2 * SK + 32;        // bytes per staged row (activations and weights)
  constexpr int RPL = 512 / SK;             // rows per wave load of a stage
  constexpr int XL = 2 * NI / RPL;          // activation loads per stage: 2 rows x 512 B each (half slices: 4 rows x 256 B)
  constexpr int WL = 16 / RPL;              // weight loads per stage (row-major layout)
  constexpr int WSTGB = 16 * XROWB;         // weight stage per wave (row-major layout)
  constexpr int R = SWIGLU ? 2 : 1;  // weight tiles (sub-units) per 16-column output tile
  constexpr int MAXU = MAXSU / R;
  constexpr int CPT = 16;            // output columns per tile
  constexpr int RS = R;              // weight rows (and fp8 row scales) per output
  constexpr int XSTAGEB = 2 * NI * XROWB;
  constexpr int NT = 64 * NW;
  using WReg = typename std::conditional<W8 && !PK, u32x2, u32x4>::type;  // one weight load per lane
  constexpr int WEB = W8 ? 1 : 2;                                       // bytes per weight element
  constexpr int WEPL = 8;                                               // weight elements per lane-load (row-major layout)
  // registers of a weight stage in lane loads (packed bf16: 32 k per load, packed fp8: 64 k; MXFP4: a cell of codes per 128 k + one
  // of scale dwords; row-major: WL)
  constexpr int NWL = W4 ? SK / W4_CELL_K + 1 : PK ? SK / (W8 ? 64 : 32) : WL;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];  // per wave: [x stage | w stage]; reused for the reduction
  __shared__ float rs_s[16 * MT];
  __shared__ float ss_s[16 * MT][NW / 2];
  __shared__ float pub_s[MT][NW][4];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  unsigned char* xst = smem + wave * (XSTAGEB + (PK ? 0 : WSTGB));
  unsigned char* wst = xst + XSTAGEB;  // (row-major layout only)
  const int nsl = (K + 255) / 256;  // 256-wide K slices; a wave takes one contiguous range of them (first_sl below)
  const int c0 = (int)blockIdx.x * cw;                 // first output column of this block
  const int cwb = min(cw, N - c0);                     // its column count (the last block may own fewer)
  const int ntile = (cwb + CPT - 1) / CPT;             // tiles, the last one possibly partial
  const int npass = (ntile + MAXU - 1) / MAXU;
  const bool do_norm = PUB || norm_w != nullptr;  // (published statistics are the RMSNorm's: a compile-time fact for those instances)
  const int lrow = lane >> (SK == 256 ? 5 : 4), lchunk = lane & (SK / 8 - 1);  // staging loads: lane -> (row of the RPL a wave load covers, 16-byte chunk of the row's 2 SK bytes)
  const int xchunk = lchunk;
  auto xrow_of = [&](int j) { return RPL * j + lrow; };

  // activation slice: XL loads covering 2*NI rows x SK k (rows past the batch re-read row B-1: their outputs are never
  // stored), plus the RMSNorm gains of the lane's chunk
  // The slices live in a register ring of XS slots (slot of slice index j: j % XS); x of slice j + XS is requested right after slice
  // j has been staged.  Vector loads return IN ORDER: with one slot, waiting for the next slice's activations also waits for every
  // weight stage requested before them -- a product whose slices are ONE weight stage (o_proj / down_proj: a single 16-column tile)
  // then never has more than one stage in flight whatever the weight ring's depth (round 6; run_pass picks XS per sub-unit count).
  constexpr int XSMAX = DEPTH;
  u32x4 xr[XSMAX][XL];
  u32x4 gr[XSMAX];
  auto load_x = [&](auto slot_c, int sl) {
    constexpr int slot = decltype(slot_c)::value < XSMAX ? decltype(slot_c)::value : 0;  // (slots >= XS are never requested: the clamp only keeps -Warray-bounds quiet about discarded calls)
    int kg = min(sl * SK + xchunk * 8, K - 8);
    asm volatile("" : "+v"(kg));  // keep the row products out of loop-invariant registers (see issue_w)
#pragma unroll
    for (int j = 0; j < XL; ++j) {
      const unsigned off = (unsigned)min(xrow_of(j), B - 1) * (unsigned)K + (unsigned)kg;
      xr[slot][j] = *reinterpret_cast<const u32x4*>(x + off);
    }
    gr[slot] = *reinterpret_cast<const u32x4*>((do_norm ? norm_w : x) + kg);  // unconditional: see the note on counted waits below
  };
  // PUB instances (the decode step's RMSNorm products): 1 / rms of the rows this lane stages (rows 2 j + lrow) in registers once the
  // statistics are known -- read from LDS inside stage_x they cost an LDS round trip + lgkmcnt(0) per row pair and slice in the K
  // loop -- and the two roundings on element PAIRS (v_pk_mul_f32, one v_cvt_pk_bf16_f32 per rounding of a pair: 8 instead of 11
  // VALU per two elements; same operations, same bits).  The other instances keep the scalar form: with bf16 weights their 8-row
  // residual kernels are at the register limit and the extra live values spilled (o / down 9.2 / 22.6 -> 9.9 / 24.4 us, round 6).
  constexpr bool REGNORM = PUB && NI <= 4;  // (16 staged rows: the registers are not there either)
  float rsr[REGNORM ? XL : 1];
  auto load_rs = [&]() {
    if constexpr (REGNORM) {
#pragma unroll
      for (int j = 0; j < XL; ++j) rsr[j] = rs_s[xrow_of(j)];
    }
  };
  auto stage_x = [&](auto slot_c, int sl, bool valid) __attribute__((always_inline)) {
    constexpr int slot = decltype(slot_c)::value;
    const bool kvalid = valid && sl * SK + xchunk * 8 < K;
#pragma unroll
    for (int j = 0; j < XL; ++j) {
      u32x4 v = xr[slot][j];
      if (do_norm) {
        if constexpr (REGNORM) {
          const float rsj = rsr[j];
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            // weight * hidden.to(dtype): two roundings, like the GEMV prologue
            f32x2 xv = {bf16lo(v[q]), bf16hi(v[q])};
            xv = xv * f32x2{rsj, rsj};
            const unsigned int hb = __builtin_bit_cast(unsigned int, __builtin_convertvector(xv, bf16x2));
            f32x2 o = f32x2{bf16lo(gr[slot][q]), bf16hi(gr[slot][q])} * f32x2{bf16lo(hb), bf16hi(hb)};
            v[q] = __builtin_bit_cast(unsigned int, __builtin_convertvector(o, bf16x2));
          }
        } else {
          const float rsj = rs_s[xrow_of(j)];
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const float lo = bf16lo(gr[slot][q]) * rnd<bf16_t>(bf16lo(v[q]) * rsj);
            const float hi = bf16hi(gr[slot][q]) * rnd<bf16_t>(bf16hi(v[q]) * rsj);
            bf16x2 p;
            p[0] = (bf16_t)lo;
            p[1] = (bf16_t)hi;
            v[q] = __builtin_bit_cast(unsigned int, p);
          }
        }
      }
      if (!kvalid) v = u32x4{0u, 0u, 0u, 0u};  // k past K contributes zeros (the weight loads there are clamped)
      *reinterpret_cast<u32x4*>(xst + xrow_of(j) * XROWB + xchunk * 16) = v;
    }
  };

  // weight stage of sub-unit su of (pass, slice): 8 loads, each 2 rows x 512 contiguous bytes (fp8: 2 rows x 256 bytes)
  // Every load inside the K loop is issued UNCONDITIONALLY: behind a branch the compiler cannot count the loads in flight, waits
  // for vmcnt(0) in front of the LDS writes and so drains the prefetched stage every step -- one full memory latency per stage,
  // which is what bounded this kernel before.  The loads are BUFFER loads on a descriptor of the tile's valid rows: what must not
  // be fetched (a stage past the wave's last slice, rows past the tile's last one, k past K) is pushed out of the descriptor's
  // range and comes back as zeros without a memory access -- no per-load select, and the per-lane part of the address is eight
  // kernel-constant offsets (row 2j + lrow, chunk lchunk) plus one slice offset per stage: 12 VALU per stage where the
  // flat-address form spent 45 (the ISA of round 2's kernel: 126 v_cndmask + 104 shifts / adds per 8 stages).
  unsigned wrow_off[WL];
#pragma unroll
  for (int j = 0; j < WL; ++j) wrow_off[j] = ((unsigned)(RPL * j + lrow) * (unsigned)K + (unsigned)lchunk * WEPL) * WEB;
  constexpr unsigned W_OUT_OF_RANGE = 0x10000000u;  // > any descriptor range (16 rows x K x 2 bytes), no 32-bit wrap when added
  auto issue_w = [&](WReg* w, int pass, int sl, int su, bool ok) {
    const int cb = c0 + (pass * MAXU + su / R) * CPT;  // first column of the tile
    const int nrow = min(c0 + cwb - cb, 16);  // valid rows of the tile (16 except in the block's last tile)
    if constexpr (W4) {
      // cell (granule, 128 k) of the packed MXFP4 array: [g][row in granule][16 code bytes] | [row in granule][4 scale bytes]; lane
      // (c, g) reads row c % gr of the tile's granule c / gr.  Loads pushed out of the descriptor's range return code 0, scale 0: +0
      const unsigned cellb = 68u << gr_shift;                      // bytes of a cell
      const unsigned gstride = (unsigned)(K / W4_CELL_K) * cellb;  // bytes of a granule
      const unsigned char* base = reinterpret_cast<const unsigned char*>(Wv) + (size_t)((cb + (su % R) * N) >> gr_shift) * gstride;
      const int ngran = (nrow + (1 << gr_shift) - 1) >> gr_shift;
      const __amdgpu_buffer_rsrc_t rs =
          __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned char*>(base), 0, nrow > 0 ? ngran * (int)gstride : 0, 0x00020000);
      const unsigned c = lane & 15, g = lane >> 4, cg = c & ((1u << gr_shift) - 1), goff = (c >> gr_shift) * gstride;
      const unsigned code_off = goff + ((g << gr_shift) + cg) * 16u, sc_off = goff + (64u << gr_shift) + cg * 4u;
      const unsigned so = ok ? (unsigned)(sl * (SK / W4_CELL_K)) * cellb : W_OUT_OF_RANGE;
      unsigned int sc[SK / W4_CELL_K];
#pragma unroll
      for (int j = 0; j < SK / W4_CELL_K; ++j) {
        // cells past K (last slice of a K that is no multiple of 256) leave the range
        const unsigned oj = sl * SK + j * W4_CELL_K < K ? so + j * cellb : W_OUT_OF_RANGE;
        sc[j] = __builtin_amdgcn_raw_buffer_load_b32(rs, (int)(sc_off + oj), 0, 2);
        w[j] = __builtin_bit_cast(WReg, __builtin_amdgcn_raw_buffer_load_b128(rs, (int)(code_off + oj), 0, 2));  // aux 2 = nt
        __builtin_amdgcn_sched_barrier(0);
      }
      w[SK / W4_CELL_K] = WReg{sc[0], sc[SK / W4_CELL_K - 1], 0u, 0u};  // (one cell per stage: the second dword is unused)
    } else if constexpr (PK) {
      // granule (cb + (su % R) N) / gr of the packed array (tile starts, block widths and the stacked half's row count are multiples
      // of gr; rows past the matrix inside its last granule are zeros in the array).  Lane (c = lane & 15, g = lane >> 4) reads row
      // c % gr of the tile's granule c / gr: 16 bytes per k block, the k blocks of a granule gr x 64 bytes apart
      const unsigned gstride = (unsigned)K * WEB << gr_shift;  // bytes of a granule
      const unsigned char* base = reinterpret_cast<const unsigned char*>(Wv) + ((size_t)cb + (size_t)(su % R) * N) * K * WEB;
      const int ngran = (nrow + (1 << gr_shift) - 1) >> gr_shift;
      const __amdgpu_buffer_rsrc_t rs =
          __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned char*>(base), 0, nrow > 0 ? ngran * (int)gstride : 0, 0x00020000);
      constexpr int KBLK = W8 ? 64 : 32;  // k per load
      const unsigned c = lane & 15, g = lane >> 4, kbs = 64u << gr_shift;  // bytes of a (granule, k block)
      const unsigned lane_off = (c >> gr_shift) * gstride + ((g << gr_shift) + (c & ((1u << gr_shift) - 1))) * 16u;
      const unsigned so = ok ? lane_off + (unsigned)(sl * (SK / KBLK)) * kbs : W_OUT_OF_RANGE;
#pragma unroll
      for (int j = 0; j < NWL; ++j) {
        // k blocks past K (last slice of a K that is no multiple of 256) leave the range
        const unsigned oj = sl * SK + j * KBLK < K ? so + j * kbs : W_OUT_OF_RANGE;
        w[j] = __builtin_bit_cast(WReg, __builtin_amdgcn_raw_buffer_load_b128(rs, (int)oj, 0, 2));  // aux 2 = nt
        __builtin_amdgcn_sched_barrier(0);
      }
    } else {
      const unsigned char* base = reinterpret_cast<const unsigned char*>(Wv) + ((size_t)cb + (size_t)(su % R) * N) * K * WEB;
      const __amdgpu_buffer_rsrc_t rs =
          __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned char*>(base), 0, nrow > 0 ? nrow * K * WEB : 0, 0x00020000);
      // slice offset; lanes whose k lies past K (last slice of a K that is no multiple of 256) leave the range too
      const unsigned so = (ok ? (unsigned)(sl * SK) * WEB : W_OUT_OF_RANGE) + (sl * SK + lchunk * WEPL < K ? 0u : W_OUT_OF_RANGE);
#pragma unroll
      for (int j = 0; j < WL; ++j) {
        if constexpr (W8) w[j] = __builtin_bit_cast(WReg, __builtin_amdgcn_raw_buffer_load_b64(rs, (int)(wrow_off[j] + so), 0, 2));
        else w[j] = __builtin_bit_cast(WReg, __builtin_amdgcn_raw_buffer_load_b128(rs, (int)(wrow_off[j] + so), 0, 2));  // aux 2 = nt
        __builtin_amdgcn_sched_barrier(0);
      }
    }
  };
  // 8 fp8 -> 8 bf16 (every e4m3 value is exactly representable in bf16)
  auto widen = [&](const u32x2& r) -> u32x4 {
    u32x4 o;
#pragma unroll
    for (int h = 0; h < 2; ++h) {  // v_cvt_scalef32_pk_bf16_fp8 (gfx950): two fp8 -> packed bf16x2 in one instruction, scale 1
      o[2 * h] = __builtin_bit_cast(unsigned int, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(r[h], 1.0f, false));
      o[2 * h + 1] = __builtin_bit_cast(unsigned int, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(r[h], 1.0f, true));
    }
    return o;
  };
  // what a staged weight load leaves in LDS: bf16 (row-major layout)
  auto staged = [&](const WReg& r) -> u32x4 {
    if constexpr (W8 && !PK) return widen(r);
    else return r;
  };
  // packed layout: the B fragment of k step s of a stage, straight from the stage's registers
  auto pk_frag = [&](const WReg* w, int s) -> bf16x8 {
    if constexpr (!PK) return bf16x8{};
    else if constexpr (W4) {
      // k step s: dword s % 4 of cell s / 4, scaled by 2^(byte s % 4 of the cell's scale dword - 127) as the fp32 `byte << 23`
      const unsigned int word = w[s >> 2][s & 3];
      const float sc = __uint_as_float(((w[SK / W4_CELL_K][s >> 2] >> (8 * (s & 3))) & 0xffu) << 23);
      u32x4 o;
      o[0] = __builtin_bit_cast(unsigned int, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(word, sc, 0));
      o[1] = __builtin_bit_cast(unsigned int, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(word, sc, 1));
      o[2] = __builtin_bit_cast(unsigned int, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(word, sc, 2));
      o[3] = __builtin_bit_cast(unsigned int, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(word, sc, 3));
      return __builtin_bit_cast(bf16x8, o);
    } else if constexpr (W8) return __builtin_bit_cast(bf16x8, widen(u32x2{w[s >> 1][2 * (s & 1)], w[s >> 1][2 * (s & 1) + 1]}));
    else return __builtin_bit_cast(bf16x8, w[s]);
  };

  // A wave's K slices are ONE contiguous range of the rows (round 3): interleaved over the waves (wave, wave + NW, ...: the first
  // version) every 512-byte piece of a weight row was fetched by a different wave at a different time -- the same DRAM pages
  // opened again and again; contiguous ranges stream 5 - 6 % faster at 4 / 8 bf16 rows, 2.5 % at 8 fp8 rows
  // (profiles/r03_skinny_contig.txt).
  const int per_wave = (nsl + NW - 1) / NW, first_sl = wave * per_wave;
  const int cnt = HS * max(0, min(per_wave, nsl - first_sl));  // stages of this wave: its slices [first_sl, first_sl + cnt / HS)
  auto sl_of = [&](int i) { return HS * first_sl + i; };
  load_x(std::integral_constant<int, 0>{}, sl_of(0));
  bool x0_ready = true;  // slot 0 holds (a request for) the first slice of the pass about to start

  // PRE: the block's first weight stage is requested before its RMSNorm statistics are reduced.  Measured per decode step
  // (profiles/r02_skinny_ab.txt, section 6): 5-8 rows bf16 -1.8 %, 3-4 rows bf16 +-0, fp8 +0.8..1 % -> bf16 only;
  // 16 staged rows: the registers are not there
  constexpr bool PRE = !W8 && NI == 4;

  // ---- RMSNorm statistics of every batch row (LlamaRMSNorm: fp32 mean of squares over K) ----
  // `between` runs once, after the statistics' first batch of loads has been issued and before it is reduced
  auto rms_stats = [&](auto&& between) {
    constexpr int HT = NT / 2;                      // threads per row parity
    constexpr int UF = (PRE && NI >= 4 ? 8 : 16) / NI;  // loads in flight per thread (8 when a weight stage is in flight too)
    const int half = tid / HT, kc = tid % HT;       // thread -> rows {2i + half}, chunks kc, kc + HT, ...
    float ss[NI];
#pragma unroll
    for (int i = 0; i < NI; ++i) ss[i] = 0.f;
    const int nch = K >> 3;
    for (int c0 = 0; c0 < nch; c0 += UF * HT) {
      u32x4 v[UF][NI];
#pragma unroll
      for (int u = 0; u < UF; ++u)
#pragma unroll
        for (int i = 0; i < NI; ++i) {
          const int b = min(2 * i + half, B - 1);
          const int c = min(c0 + u * HT + kc, nch - 1);
          v[u][i] = *reinterpret_cast<const u32x4*>(x + (size_t)b * K + (size_t)c * 8);
        }
      if (c0 == 0) {
        __builtin_amdgcn_sched_barrier(0);
        between();
        __builtin_amdgcn_sched_barrier(0);
      }
#pragma unroll
      for (int u = 0; u < UF; ++u) {
        const bool ok = c0 + u * HT + kc < nch;
#pragma unroll
        for (int i = 0; i < NI; ++i) {
          float s = 0.f;
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const float lo = bf16lo(v[u][i][q]), hi = bf16hi(v[u][i][q]);
            s += lo * lo + hi * hi;
          }
          ss[i] += ok ? s : 0.f;
        }
      }
    }
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      const float t = wave_sum(ss[i]);
      if (lane == 0) ss_s[2 * i + half][wave % (NW / 2)] = t;
    }
    __syncthreads();
    if (tid < 2 * NI) {
      float t = 0.f;
#pragma unroll
      for (int k = 0; k < NW / 2; ++k) t += ss_s[tid][k];
      rs_s[tid] = rsqrtf(t / (float)K + norm_eps);
    }
    __syncthreads();
  };

  // ---- the same statistics from the producer's published partial sums (PUB) ----
  // wave w owns rows w, w + NW, ...; `between` runs after the loads have been requested (the first weight stage queues behind them)
  auto pub_stats = [&](auto&& between) {
    constexpr int RPW = (2 * NI + NW - 1) / NW;
    constexpr int RG = RPW > 4 ? 4 : RPW;  // rows in flight per wave (a wide pass of a 4-wave block: two groups of 4)
    static_assert(RPW % RG == 0, "row groups");
#pragma unroll
    for (int j0 = 0; j0 < RPW; j0 += RG) {
      f32x4 sv[RG][2];
#pragma unroll
      for (int j = 0; j < RG; ++j) {
        const float* p = ss_in + (size_t)min(wave + (j0 + j) * NW, B - 1) * SRGPT_ROWSS_STRIDE + lane * 8;
        sv[j][0] = *reinterpret_cast<const f32x4*>(p);
        sv[j][1] = *reinterpret_cast<const f32x4*>(p + 4);
      }
      if (j0 == 0) {
        __builtin_amdgcn_sched_barrier(0);
        between();
        __builtin_amdgcn_sched_barrier(0);
      }
#pragma unroll
      for (int j = 0; j < RG; ++j) {
        float t = ((sv[j][0][0] + sv[j][0][1]) + (sv[j][0][2] + sv[j][0][3])) + ((sv[j][1][0] + sv[j][1][1]) + (sv[j][1][2] + sv[j][1][3]));
        t = wave_sum(t);
        if (lane == 0 && wave + (j0 + j) * NW < 2 * NI) rs_s[wave + (j0 + j) * NW] = rsqrtf(t / (float)K + norm_eps);
      }
    }
    __syncthreads();
  };
  float pub_acc = 0.f;  // ss_out: sum of squares of this thread's output elements (all of one batch row: see the epilogue)
  float pub_acc1 = 0.f;  // ... in the second M tile of a wide pass

  // one pass over K for NSU sub-units
  auto run_pass = [&](auto nsu_c, int pass, int nu) {
    constexpr int NSU = decltype(nsu_c)::value;
    constexpr int NS = SK / 32;           // MFMA k steps per stage
    constexpr int FS = NI >= 8 ? 2 : FS_MAX;  // k steps whose fragments are read together (16 staged rows: fewer, registers)
    constexpr bool TWO_ACC = NI < 8;  // even / odd k steps on separate accumulators (16 staged rows: the registers are not there)
    // slots of the activation ring (see load_x): as many slices ahead as the weight ring reaches
    // (fp8 only: with bf16 weights a stage is twice the registers and the 8-row single-tile kernel spills under a second slot --
    //  o / down 9.2 / 22.6 -> 9.9 / 24.4 us at 8 bf16 rows, profiles/r06_skinny_norm_staging.txt)
    // (MXFP4: a stage is 10 registers, the slots are there)
    // (32 staged rows: a slot is 64 registers, one slot)
    constexpr int XS = (!W8 && !W4) || MT == 2 ? 1 : NSU == 1 ? DEPTH : (NSU == 2 && DEPTH == 4 ? 2 : 1);
    static_assert(DEPTH % XS == 0, "the slot of a slice must be a compile-time function of its place in the trip");
    if (!x0_ready) load_x(std::integral_constant<int, 0>{}, sl_of(0));
    if constexpr (XS > 1) load_x(std::integral_constant<int, 1>{}, sl_of(min(1, max(cnt - 1, 0))));
    if constexpr (XS > 2) load_x(std::integral_constant<int, 2>{}, sl_of(min(2, max(cnt - 1, 0))));
    if constexpr (XS > 3) load_x(std::integral_constant<int, 3>{}, sl_of(min(3, max(cnt - 1, 0))));
    x0_ready = XS == 1;  // a one-slot pass leaves the next pass's first slice requested
    f32x4 acc[NSU * MT], acc2[TWO_ACC ? NSU : 1];  // acc[mt NSU + su]: one accumulator per (sub-unit, M tile)
#pragma unroll
    for (int su = 0; su < NSU * MT; ++su) acc[su] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int su = 0; su < (TWO_ACC ? NSU : 1); ++su) acc2[su] = f32x4{0.f, 0.f, 0.f, 0.f};
    // register ring of DEPTH weight stages with static slot indices (a trip = DEPTH slices x NSU stages, a multiple of
    // DEPTH): the loads of stage t+DEPTH-1 are issued before stage t is multiplied.  A stage is 8 KiB per wave (fp8: 4 KiB).
    WReg wb[DEPTH][NWL];
    // epilogue operands that do not depend on the products -- row scales (W8) and residual elements -- are requested up front
    // (fetched at their use they would each add a memory round trip after the last barrier of the pass), but BEHIND the first
    // weight stages and without touching their values: round 4's form, `residual ? (float)residual[i] : 0` in front of the first
    // weight request, compiled to branch -> load -> s_waitcnt vmcnt(0) -> convert per element -- o_proj and down_proj went
    // through up to four serialised memory round trips (2.7k cycles, profiles/r05_skinny_stamps.txt) before asking for a weight
    constexpr int EIT0 = ((NSU / R) * 256 + NT - 1) / NT;  // epilogue iterations per thread
    constexpr int EIT = EIT0 > 0 ? EIT0 : 1;               // (odd NSU never occurs with SwiGLU; keep the type valid)
    float pre_sc[EIT][RS];
    unsigned short pre_res[MT * EIT];  // bf16 bits
    auto load_epilogue_operands = [&]() {
      const bool has_res = !SWIGLU && residual != nullptr;
      const bf16_t* rp = has_res ? residual : x;
#pragma unroll
      for (int i = 0; i < EIT; ++i) {
        const int e = tid + i * NT;
        const int u = e >> 8, l2 = e & 63, q = (e >> 6) & 3;
        const int b = min(4 * (l2 >> 4) + q, B - 1);
        const int n = min(c0 + (pass * MAXU + u) * CPT + (l2 & (CPT - 1)), c0 + cwb - 1);
#pragma unroll
        for (int r = 0; r < RS; ++r) pre_sc[i][r] = W8 ? wscale[n + r * N] : 1.f;
        pre_res[i] = *reinterpret_cast<const unsigned short*>(rp + (has_res ? (size_t)b * N + n : (size_t)0));
        if constexpr (MT == 2)
          pre_res[EIT + i] = *reinterpret_cast<const unsigned short*>(rp + (has_res ? (size_t)min(b + 16, B - 1) * N + n : (size_t)0));
      }
    };
    // pass 0: the first weight stage goes out behind the statistics' own loads (in-order return: the reduction waits for its
    // activations only), so its HBM latency overlaps the reduction and the two block barriers -- as in the GEMV's prologue
    if (PUB && pass == 0) {
      pub_stats([&]() { issue_w(wb[0], 0, sl_of(0), 0, cnt > 0); });
      load_rs();
    } else if (PRE && pass == 0 && do_norm) {
      rms_stats([&]() { issue_w(wb[0], 0, sl_of(0), 0, cnt > 0); });
      load_rs();
    } else {
      issue_w(wb[0], pass, sl_of(0), 0, cnt > 0);
    }
#pragma unroll
    for (int f = 1; f < DEPTH - 1; ++f)
      issue_w(wb[f % DEPTH], pass, sl_of(f / NSU), f % NSU, f / NSU < cnt);
    __builtin_amdgcn_sched_barrier(0);
    load_epilogue_operands();
    __builtin_amdgcn_sched_barrier(0);
    // one slice (h-th of the trip that starts at slice index i): NSU stages
    // activation fragments of a slice held across its sub-units where the registers are there (fp8 weights: the stage ring is
    // half as wide; bf16 weights: the 4-row variant only)
    constexpr bool XREUSE = NSU >= 2 && (W8 ? NI <= 4 : NI == 2);
    auto slice = [&](int i, auto h_c) {
      constexpr int h = decltype(h_c)::value;
      const int sl = sl_of(i + h);
      bf16x8 xall[XREUSE ? NS : 1];
      {
#pragma unroll
          for (int su = 0; su < NSU; ++su) {
            const int cur = (h * NSU + su) % DEPTH;
            const int fn = h * NSU + su + DEPTH - 1;  // stage to prefetch, relative to this trip
            issue_w(wb[fn % DEPTH], pass, sl_of(i + fn / NSU), fn % NSU, i + fn / NSU < cnt);
            if (su == 0) {
              stage_x(std::integral_constant<int, h % XS>{}, sl, true);
              if constexpr (XS == 1) load_x(std::integral_constant<int, 0>{}, i + h + 1 < cnt ? sl_of(i + h + 1) : sl_of(0));  // next slice, or the first one of the next pass
              else load_x(std::integral_constant<int, h % XS>{}, sl_of(min(i + h + XS, cnt - 1)));  // XS slices ahead (past the end: a valid slice, never staged)
            }
            if constexpr (!PK) {
#pragma unroll
              for (int j = 0; j < WL; ++j) *reinterpret_cast<u32x4*>(wst + (RPL * j + lrow) * XROWB + lchunk * 16) = staged(wb[cur][j]);
            }
            __builtin_amdgcn_wave_barrier();
            // The fragment reads of FS k steps are issued together in front of their MFMAs, which alternate between two
            // accumulators.  Left to the compiler the unrolled loop became read -> wait -> MFMA per k step on ONE accumulator: a
            // full LDS latency per step, ~1.5k cycles per stage and sub-unit -- the kernel was bound by that, not by HBM.
            const int xrow = MT == 2 ? (lane & 15) : lane & (2 * NI - 1);  // rows past the staged ones alias valid rows: their outputs are never stored
            if constexpr (XREUSE) {
              // the activation fragments of the slice are the same for all of its sub-units: read once, kept in registers
              if (su == 0) {
#pragma unroll
                for (int s = 0; s < NS; ++s) xall[s] = *reinterpret_cast<const bf16x8*>(xst + xrow * XROWB + (4 * s + (lane >> 4)) * 16);
              }
            }
#pragma unroll
            for (int s0 = 0; s0 < NS; s0 += FS) {
              bf16x8 xf[FS];
              bf16x8 xf1[MT == 2 ? FS : 1];  // the second M tile's
              bf16x8 wfr[FS];
#pragma unroll
              for (int t = 0; t < FS; ++t) {
                const int s = s0 + t;
                if constexpr (XREUSE) xf[t] = xall[s];
                else xf[t] = *reinterpret_cast<const bf16x8*>(xst + xrow * XROWB + (4 * s + (lane >> 4)) * 16);
                if constexpr (MT == 2) xf1[t] = *reinterpret_cast<const bf16x8*>(xst + (xrow + 16) * XROWB + (4 * s + (lane >> 4)) * 16);
                if constexpr (PK) wfr[t] = pk_frag(wb[cur], s);
                else wfr[t] = *reinterpret_cast<const bf16x8*>(wst + (lane & 15) * XROWB + (4 * s + (lane >> 4)) * 16);
              }
              __builtin_amdgcn_sched_barrier(0);
#pragma unroll
              for (int t = 0; t < FS; ++t) {
                const bf16x8 wf = wfr[t];
                // D[batch row][weight row] += x[batch row][k] * W[weight row][k]
                if (TWO_ACC && (t & 1)) acc2[TWO_ACC ? su : 0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xf[t], wf, acc2[TWO_ACC ? su : 0], 0, 0, 0);
                else acc[su] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xf[t], wf, acc[su], 0, 0, 0);
                if constexpr (MT == 2) acc[NSU + su] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xf1[t], wf, acc[NSU + su], 0, 0, 0);
              }
              __builtin_amdgcn_sched_barrier(0);
            }
            __builtin_amdgcn_wave_barrier();
          }
      }
    };
    // full trips run branch-free; the last cnt % DEPTH slices are guarded (nothing is left to prefetch behind them, so the
    // conservative waits the guard brings cost nothing)
    int i = 0;
    for (; i + DEPTH <= cnt; i += DEPTH) {
      slice(i, std::integral_constant<int, 0>{});
      if constexpr (DEPTH > 1) slice(i, std::integral_constant<int, 1>{});
      if constexpr (DEPTH > 2) slice(i, std::integral_constant<int, 2>{});
      if constexpr (DEPTH > 3) slice(i, std::integral_constant<int, 3>{});
    }
    if (i < cnt) slice(i, std::integral_constant<int, 0>{});
    if constexpr (DEPTH > 2)
      if (i + 1 < cnt) slice(i, std::integral_constant<int, 1>{});
    if constexpr (DEPTH > 3)
      if (i + 2 < cnt) slice(i, std::integral_constant<int, 2>{});
    static_assert(DEPTH >= 2 && DEPTH <= 4, "ring depth");

    // ---- cross-wave reduction (fixed order) + epilogue ----
    __syncthreads();
    float* redf = reinterpret_cast<float*>(smem);  // [NW waves][MT M tiles][MAXSU][64 lanes][4]
#pragma unroll
    for (int su = 0; su < NSU; ++su) *reinterpret_cast<f32x4*>(redf + ((wave * MT * MAXSU + su) * 64 + lane) * 4) = TWO_ACC ? acc[su] + acc2[TWO_ACC ? su : 0] : acc[su];
    if constexpr (MT == 2) {
#pragma unroll
      for (int su = 0; su < NSU; ++su) *reinterpret_cast<f32x4*>(redf + (((wave * MT + 1) * MAXSU + su) * 64 + lane) * 4) = acc[NSU + su];
    }
    __syncthreads();
    // (a wide pass: the iterations of M tile 0, rows 0 .. 15, then those of M tile 1)
#pragma unroll
    for (int im = 0; im < MT * EIT; ++im) {
      const int mt = im / EIT, i = im % EIT;
      const int e = tid + i * NT;
      if (e >= (NSU / R) * 256) {
        if constexpr (MT == 1) break;
        else continue;
      }
      const int u = e >> 8, l2 = e & 63, q = (e >> 6) & 3;
      const int b = 16 * mt + 4 * (l2 >> 4) + q;
      const int n = c0 + (pass * MAXU + u) * CPT + (l2 & 15);
      float a[RS];
#pragma unroll
      for (int r = 0; r < RS; ++r) {
        float t = 0.f;
#pragma unroll
        for (int wv = 0; wv < NW; ++wv) t += redf[(((wv * MT + mt) * MAXSU + u * R + r) * 64 + l2) * 4 + q];
        if (W8) t *= pre_sc[i][r];
        a[r] = t;
      }
      if (b < B && n < c0 + cwb) {
        if (SWIGLU) {
          const float g = rnd<bf16_t>(a[0]), up = rnd<bf16_t>(a[RS - 1]);
          reinterpret_cast<bf16_t*>(out)[(size_t)b * N + n] = (bf16_t)(rnd<bf16_t>(silu(g)) * up);
        } else {
          float v = rnd<bf16_t>(a[0]);
          if (residual) v = rnd<bf16_t>(__uint_as_float((unsigned int)pre_res[mt * EIT + i] << 16) + v);
          if (MT == 2 && mt == 1) pub_acc1 = fmaf(v, v, pub_acc1);
          else pub_acc = fmaf(v, v, pub_acc);
          if (out_f32)
            reinterpret_cast<float*>(out)[(size_t)b * N + n] = v;
          else
            reinterpret_cast<bf16_t*>(out)[(size_t)b * N + n] = (bf16_t)v;
        }
      }
    }
    __syncthreads();  // the reduction buffer aliases the wave-private stages of the next pass
  };

  if (!PUB && !PRE && do_norm) {
    rms_stats([]() {});
    load_rs();
  }
  for (int pass = 0; pass < npass; ++pass) {
    int nu = 0;
#pragma unroll
    for (int u = 0; u < MAXU; ++u) nu += (pass * MAXU + u < ntile) ? 1 : 0;
    if (nu == 0) break;  // uniform per block; later passes are empty too
    switch (nu * R) {
      case 1: run_pass(std::integral_constant<int, 1>{}, pass, nu); break;
      case 2: run_pass(std::integral_constant<int, 2>{}, pass, nu); break;
      case 3: run_pass(std::integral_constant<int, 3>{}, pass, nu); break;
      default: run_pass(std::integral_constant<int, 4>{}, pass, nu); break;
    }
  }
  if constexpr (!SWIGLU) {
    if (ss_out != nullptr) {
      // epilogue element e = tid + i NT sits in batch row 4 (lane >> 4) + (wave & 3) whatever i and the pass are: a thread's pub_acc
      // belongs to ONE row, and the 16 lanes of a DPP row hold that row's 16 columns of every tile; waves w and w + 4 (8-wave blocks)
      // hold different tiles of the same rows: added in wave order through LDS
      float tot = lanes_sum<16>(pub_acc);
      if constexpr (NW > 4) {
        if ((lane & 15) == 0) pub_s[0][wave][lane >> 4] = tot;
        __syncthreads();
        if (wave < 4) {
          tot = 0.f;
#pragma unroll
          for (int wv = 0; wv < NW; wv += 4) tot += pub_s[0][wave + wv][lane >> 4];
        }
      }
      const int b = 4 * (lane >> 4) + wave;
      if (wave < 4 && (lane & 15) == 0 && b < B) {
        float* row = ss_out + (size_t)b * SRGPT_ROWSS_STRIDE;
        row[blockIdx.x] = tot;
        for (int sidx = (int)blockIdx.x + (int)gridDim.x; sidx < SRGPT_ROWSS_STRIDE; sidx += (int)gridDim.x) row[sidx] = 0.f;
      }
      if constexpr (MT == 2) {  // the second M tile of a wide pass: rows 16 + ..., the same sums in the same order
        float tot1 = lanes_sum<16>(pub_acc1);
        if constexpr (NW > 4) {
          if ((lane & 15) == 0) pub_s[1][wave][lane >> 4] = tot1;
          __syncthreads();
          if (wave < 4) {
            tot1 = 0.f;
#pragma unroll
            for (int wv = 0; wv < NW; wv += 4) tot1 += pub_s[1][wave + wv][lane >> 4];
          }
        }
        if (wave < 4 && (lane & 15) == 0 && b + 16 < B) {
          float* row = ss_out + (size_t)(b + 16) * SRGPT_ROWSS_STRIDE;
          row[blockIdx.x] = tot1;
          for (int sidx = (int)blockIdx.x + (int)gridDim.x; sidx < SRGPT_ROWSS_STRIDE; sidx += (int)gridDim.x) row[sidx] = 0.f;
        }
      }
    }
  }
}

static_assert(GEMV_SKINNY_ROW_BYTES == WROWB && 16 * GEMV_SKINNY_ROW_BYTES == WSTAGEB && GEMV_SKINNY_SUBUNITS == MAXSU,
              "gemv_route.h sizes the kernel's LDS: K loop stages | reduction buffer");

}  // namespace

// One weight pass of up to 16 rows (a wide chunk: 17 - 32) on the MFMA kernel (GEMV_SKINNY of gemv_route.h), entered from srgpt_decode_product (gemv.hip);
// bf16 or fp8 weights.  packed: 0 = row-major W [N][K]; 4 / 8 / 16 = the packed decode layout with granules of that many rows
// (srgpt_pack_decode_weights); ss_in / ss_out: the rows' statistics tables (see skinny_kernel).  w4 (from srgpt_gemv_w4p,
// gemv_w4p.hip): W is a packed MXFP4 array (srgpt_pack_mxfp4), packed = its granule rows
int srgpt_skinny_launch(const DecodeProduct& p, hipStream_t s) {
  const int packed = p.packed, kblock = p.w4 ? W4_CELL_K : p.fp8 ? 64 : 32;
  SRGPT_CHECK(!p.w4 || (packed == W4_GRANULE_ROWS && !p.fp8), SRGPT_ERR_ARG, "skinny: MXFP4 weights come in packed granules of %d rows",
              W4_GRANULE_ROWS);
  SRGPT_CHECK(packed == 0 || packed == 4 || packed == 8 || packed == 16, SRGPT_ERR_ARG, "skinny: packed layout granule %d (0, 4, 8 or 16)", packed);
  SRGPT_CHECK(p.batch >= 1 && p.batch <= GEMV_WIDE_ROWS, SRGPT_ERR_ARG, "skinny: batch %d outside 1..%d", p.batch, GEMV_WIDE_ROWS);
  SRGPT_CHECK(p.K % 8 == 0 && p.K >= 8, SRGPT_ERR_ARG, "skinny: K=%d must be a multiple of 8", p.K);
  SRGPT_CHECK(!p.ss_in || p.norm_w, SRGPT_ERR_ARG, "skinny: published row statistics are the RMSNorm's input (norm_w is NULL)");
  SRGPT_CHECK(!p.ss_out || (!p.swiglu && !p.out_f32), SRGPT_ERR_ARG, "skinny: row statistics are published for plain bf16 outputs only");
  // 17 - 32 rows: a chunk of gemv_wide_route (the other routes cut a call into passes of 16)
  const GemvSkinnyLaunch l = p.batch > 16 ? gemv_wide_launch(p.batch, p.N, p.norm_w != nullptr, p.ss_in != nullptr, packed, srgpt_device_cus())
                                          : gemv_skinny_launch(p.batch, p.N, p.norm_w != nullptr, p.ss_in != nullptr, packed, srgpt_device_cus());
  SRGPT_CHECK(!p.ss_out || l.grid <= SRGPT_ROWSS_STRIDE, SRGPT_ERR_UNSUPPORTED, "skinny: %d blocks do not fit the %d row-statistics slots",
              l.grid, SRGPT_ROWSS_STRIDE);
  SRGPT_CHECK(!packed || (p.K % kblock == 0 && (!p.swiglu || p.N % packed == 0)), SRGPT_ERR_UNSUPPORTED,
              "skinny: the packed weight layout needs K %% %d == 0 (K = %d)%s", kblock, p.K, p.swiglu ? " and whole granules per half" : "");
  const auto flag = [](bool v, const char* what, auto&& f) { return srgpt_switch<false, true>(v, what, f); };
  SRGPT_TRY((flag(p.swiglu != 0, "SWIGLU", [&](auto sw_c) {
    return srgpt_switch<2, 4, 8, 16>(l.NI, "NI", [&](auto ni_c) {
      return srgpt_switch<4, 8>(l.NW, "NW", [&](auto nw_c) {
        return flag(p.fp8 != 0, "W8", [&](auto w8_c) {
          return flag(l.PUB, "PUB", [&](auto pub_c) {
            return flag(l.PK, "PK", [&](auto pk_c) {
              return flag(p.w4 != 0, "W4", [&](auto w4_c) {
                constexpr int NI = decltype(ni_c)::value, NW = decltype(nw_c)::value;
                constexpr bool PK = decltype(pk_c)::value, W8 = decltype(w8_c)::value, W4 = decltype(w4_c)::value;
                constexpr int LDS = NI == 16 ? gemv_wide_lds(NW, PK) : gemv_skinny_lds(NI, NW, PK);
                static_assert(LDS <= 160 * 1024, "LDS");
                static_assert(NW == 8 || 2 * LDS <= 160 * 1024, "two 4-wave blocks per CU");
                if constexpr (W4 && (!PK || W8)) {
                  return (int)SRGPT_ERR_ARG;  // (checked above: MXFP4 weights are packed and not fp8)
                } else if constexpr (NI == 16 && !gemv_wide_has_instance(W8, PK ? 16 : 0, W4)) {
                  srgpt_set_error("skinny: no wide instance for these weights (gemv_wide_route keeps them at 16 rows)");
                  return (int)SRGPT_ERR_UNSUPPORTED;
                } else {
                  constexpr auto kfn = &skinny_kernel<decltype(sw_c)::value, NI, NW, W8, decltype(pub_c)::value, PK, W4>;
                  return srgpt_launch_dyn_lds<kfn>(l.lds, dim3(l.grid), dim3(64 * NW), (size_t)l.lds, s, (const bf16_t*)p.x, p.W, p.wscale,
                                                   (const bf16_t*)p.norm_w, p.eps, (const bf16_t*)p.residual, p.out, p.batch, p.N, p.K,
                                                   p.out_f32, l.cw, p.ss_in, p.ss_out, l.gr_shift);
                }
              });
            });
          });
        });
      });
    });
  })));
  SRGPT_LAUNCH_CHECK();
  return SRGPT_OK;
}

// Decode-path product with fp8 (OCP e4m3fn) weights and one fp32 scale per weight row, bf16 activations (W8A16):
// out[b, n] = bf16( (sum_k x[b, k] * fp8(W8[n, k])) * wscale[n] ), same fusions as srgpt_gemv.  Any batch size
// (16 rows per weight pass).
extern "C" int srgpt_gemv_w8(const void* x, const void* W8, const float* wscale, const void* norm_w, float norm_eps,
                             const void* residual, void* out, int batch, int N, int K, int swiglu, int out_f32,
                             srgpt_stream_t stream) {
  SRGPT_CHECK(x && W8 && wscale && out, SRGPT_ERR_ARG, "srgpt_gemv_w8: null pointer");
  SRGPT_CHECK(N > 0 && K > 0 && batch > 0, SRGPT_ERR_ARG, "srgpt_gemv_w8: bad shape");
  SRGPT_CHECK(K % 8 == 0, SRGPT_ERR_ARG, "srgpt_gemv_w8: K=%d must be a multiple of 8", K);
  SRGPT_CHECK(!(swiglu && (residual || out_f32)), SRGPT_ERR_ARG, "srgpt_gemv_w8: swiglu excludes residual/out_f32");
  return srgpt_decode_product(DecodeProduct{x, W8, wscale, norm_w, norm_eps, residual, out, batch, N, K, swiglu, out_f32, SRGPT_BF16, 1,
                                            nullptr, nullptr, 0},
                              as_stream(stream));
}

// ---- the packed decode layout (include/srgpt.h, ABI 9) ----
namespace {
// one thread per 16 output bytes: (granule, k block, g, row in granule)
__global__ __launch_bounds__(256) void pack_decode_kernel(const unsigned char* __restrict__ W, unsigned char* __restrict__ out, int N, int K,
                                                          int eb, int rows, long long n16) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n16) return;
  const int kblock = 32 * (2 / eb);           // k per 16-byte lane load: 64 (fp8) / 32 (bf16)
  const int nkb = K / kblock;
  const int r = (int)(i % rows), g = (int)(i / rows % 4);
  const long long t = i / (4 * rows);
  const int kb = (int)(t % nkb);
  const long long n = t / nkb * rows + r;
  u32x4 v = {0u, 0u, 0u, 0u};
  if (n < N) {
    const unsigned char* src = W + ((size_t)n * K + (size_t)kb * kblock + 8 * g) * eb;
    if (eb == 2) {
      v = *reinterpret_cast<const u32x4*>(src);                                    // 8 bf16: k = 32 kb + 8 g .. + 8
    } else {
      const u32x2 lo = *reinterpret_cast<const u32x2*>(src), hi = *reinterpret_cast<const u32x2*>(src + 32);  // k = 64 kb (+ 32) + 8 g .. + 8
      v = u32x4{lo[0], lo[1], hi[0], hi[1]};
    }
  }
  *reinterpret_cast<u32x4*>(out + (size_t)i * 16) = v;
}
}  // namespace

extern "C" size_t srgpt_packed_bytes(int N, int K, int elem_bytes, int rows) {
  if (N <= 0 || K <= 0 || rows <= 0 || (elem_bytes != 1 && elem_bytes != 2)) return 0;
  return (size_t)((N + rows - 1) / rows) * rows * K * elem_bytes;
}

extern "C" int srgpt_pack_decode_weights(const void* W, void* out, int N, int K, int elem_bytes, int rows, srgpt_stream_t stream) {
  SRGPT_CHECK(W && out, SRGPT_ERR_ARG, "srgpt_pack_decode_weights: null pointer");
  SRGPT_CHECK(elem_bytes == 1 || elem_bytes == 2, SRGPT_ERR_ARG, "srgpt_pack_decode_weights: %d bytes per element (1: fp8, 2: bf16)", elem_bytes);
  SRGPT_CHECK(rows == 4 || rows == 8 || rows == 16, SRGPT_ERR_ARG, "srgpt_pack_decode_weights: %d rows per granule (4, 8 or 16)", rows);
  SRGPT_CHECK(N > 0 && K > 0 && K % (elem_bytes == 1 ? 64 : 32) == 0, SRGPT_ERR_ARG,
              "srgpt_pack_decode_weights: K=%d must be a positive multiple of %d", K, elem_bytes == 1 ? 64 : 32);
  const long long n16 = (long long)(srgpt_packed_bytes(N, K, elem_bytes, rows) / 16);
  hipLaunchKernelGGL(pack_decode_kernel, dim3((unsigned)((n16 + 255) / 256)), dim3(256), 0, as_stream(stream), (const unsigned char*)W,
                     (unsigned char*)out, N, K, elem_bytes, rows, n16);
  SRGPT_LAUNCH_CHECK();
  return SRGPT_OK;
}
