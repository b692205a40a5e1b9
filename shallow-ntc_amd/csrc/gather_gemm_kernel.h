#pragma once
// gather_gemm_kernel.h -- the one contraction kernel of the codec (the kernel TEMPLATE; instantiated per mode in gg_inst_*.hip,
// launched from gather_gemm.hip): an im2col-free, NHWC gather GEMM on
// the gfx950 fp32 matrix cores (v_mfma_f32_32x32x2_f32: exact f32 fma chain, 64 FLOP/clk/SIMD).
//
// Every Conv2D / Conv2DTranspose / SignalConv2D / GDN norm-pool on the hot path is
//     out[m, col] = sum_t sum_c x[src(m, t), c] * Wp[col][t*Cin + c]          (sntc_internal.h)
// with pixels on the MFMA row (A) side and output columns on the column (B) side.
//
// Workgroup: 256 threads = 4 waves arranged WM x WN; each wave owns TN tiles of 32x32; a K stage is 16 deep.
//   HBM/L2 -> registers: buffer_load_dwordx4 through two wave-uniform descriptors (input, packed weights) with a
//   32-bit per-lane byte offset that changes only when the tap changes and a scalar offset that walks the channel
//   slabs / K stages; rows whose source pixel falls outside the image carry an out-of-range offset and read zeros
//   from the bounds check (no branches, no 64-bit address arithmetic in the loop).  The per-lane offset of a tap is
//   base + delta with bit 31 set unless (mask & select) == select (gg_tap_rules.h): base (tap (0, 0) of the row) and mask
//   (which tap rows / columns of the row are inside the image) are made once per tile, delta and select are scalars the
//   tap walk advances with adds -- 4 vector instructions per row and stage, no multiply.  Cin % 16 != 0 (the RGB first
//   layer, reduced-width test nets) takes the dword gather path: one k column per thread, (tap, channel) advanced
//   incrementally, same bounds-check zero fill.
//   registers -> LDS: a ring of THREE 16-deep stages, 64-B rows, 16-B chunks XOR-swizzled by (row >> 2) & 3, so the
//   staging ds_write_b128 and the fragment ds_read_b128 are bank-conflict free without padding.
//   Pipeline, ONE barrier per stage: in step j a wave (1) writes stage j+2 (loaded during step j-1) into the slot that
//   held stage j-1, (2) issues the global loads of stage j+3, (3) multiplies stage j from fragments it prefetched,
//   reading the second half's fragments and then the FIRST fragments of stage j+1 under the MFMAs -- so nothing
//   waits on LDS after the barrier.  Per lane a ds_read_b128 fetches k = 8g+4h..8g+4h+3 (h = lane>>5): MFMA e of
//   k-group g sums k in {8g+e, 8g+4+e}; A and B use the same permutation, so the products pair up.
//   C/D layout: col = lane & 31, row = (reg & 3) + 8*(reg >> 2) + 4*(lane >> 5).
//
// Scheduling.  Static mode: one workgroup per (tile, K range); K ranges > 1 leave raw partial sums for
// gg_reduce_kernel (deterministic split-K for layers with few tiles per image).  Stream-K mode: as many workgroups
// as the device keeps resident each take an equal share of the launch's (tile, stage) units.  A worker whose share
// ends inside a tile computes that tile's first stages FIRST and publishes the raw accumulators; the next worker
// finishes the tile LAST, starting its fma chains from those accumulators.  Every output element is therefore the
// same k-ordered chain as in an unsplit tile: results do not depend on the worker count, the batch size or the tile
// shape, and no tile quantisation is left (2160 tiles on 768 slots used to run 3 rounds for 2.81 rounds of work).
// Between tiles the next tile's first two stages are in flight while the current tile's epilogue runs.
#include <algorithm>
#include <cstdlib>
#include <mutex>
#include <type_traits>
#include "sntc_internal.h"
#include "gg_tap_rules.h"
#include "gg_pieces.h"     // the piece walk (which stages of which tile a workgroup computes) and the stream-K hand-off

namespace sntc {

// f(integral_constant<int, HI>), f(HI - 1), ..., f(LO): stops after the first call that returns true; says whether one did
template <int HI, int LO, class F>
__device__ __forceinline__ bool first_of_desc(F&& f) {
  if constexpr (HI < LO) {
    return false;
  } else {
    if (f(std::integral_constant<int, HI>{})) return true;
    return first_of_desc<HI - 1, LO>(f);
  }
}

// f(integral_constant<int, 0>), ..., f(N - 1), every one
template <int N, int I = 0, class F>
__device__ __forceinline__ void each_of(F&& f) {
  if constexpr (I < N) {
    f(std::integral_constant<int, I>{});
    each_of<N, I + 1>(f);
  }
}

// a step's WR / LD / PF switch: an integral_constant (the steady state and the old tails: no branch) or a run-time bool
template <class T> constexpr bool gg_yes = std::is_same_v<T, std::integral_constant<bool, true>>;
template <class T>
__device__ __forceinline__ constexpr bool gg_flag(T f) {
  if constexpr (std::is_same_v<T, bool>) return f;
  else return T::value;
}

__device__ __forceinline__ f32x4 buf_load(__amdgpu_buffer_rsrc_t rsrc, unsigned voff, unsigned soff) {
  const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rsrc, (int)voff, (int)soff, 0);
  return __builtin_bit_cast(f32x4, v);
}

__device__ __forceinline__ float buf_load1(__amdgpu_buffer_rsrc_t rsrc, unsigned voff) {
  return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rsrc, (int)voff, 0, 0));
}

__device__ __forceinline__ f32x4 apply_epilogue(f32x4 v, int epi, const f32x4 rs, const float* aux, size_t idx) {
  switch (epi) {
    case SNTC_EPI_ADD: return v + rs;
    case SNTC_EPI_GATE: return rs + *reinterpret_cast<const f32x4*>(aux + idx) * v;
    case SNTC_EPI_RES_DIV: return rs / v;
    case SNTC_EPI_RES_MUL: return rs * v;
    case SNTC_EPI_RES_DIV_SQRT:
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = rs[e] / sqrtf(v[e]);
      return v;
    case SNTC_EPI_RES_MUL_SQRT:
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = rs[e] * sqrtf(v[e]);
      return v;
    case SNTC_EPI_MASK_RELU:
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = rs[e] > 0.0f ? v[e] : 0.0f;
      return v;
    case SNTC_EPI_MASK_LEAKY:
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = rs[e] >= 0.0f ? v[e] : 0.2f * v[e];
      return v;
    case SNTC_EPI_DEQUANT: {   // rs: the row load of `res` as for SNTC_EPI_ADD, holding int32 symbols; converted here.  The
      // whole vector is cast (a bit cast of one element, rs[e], reads the vector's first four bytes for every e)
      typedef int i32x4 __attribute__((ext_vector_type(4)));
      const i32x4 s = __builtin_bit_cast(i32x4, rs);
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] += (float)s[e];
      return v;
    }
    default: return v;
  }
}

__device__ __forceinline__ float apply_epilogue1(float v, int epi, const float* res, const float* aux, size_t idx) {
  switch (epi) {
    case SNTC_EPI_ADD: return v + res[idx];
    case SNTC_EPI_GATE: return res[idx] + aux[idx] * v;
    case SNTC_EPI_RES_DIV: return res[idx] / v;
    case SNTC_EPI_RES_MUL: return res[idx] * v;
    case SNTC_EPI_RES_DIV_SQRT: return res[idx] / sqrtf(v);
    case SNTC_EPI_RES_MUL_SQRT: return res[idx] * sqrtf(v);
    case SNTC_EPI_MASK_RELU: return res[idx] > 0.0f ? v : 0.0f;
    case SNTC_EPI_MASK_LEAKY: return res[idx] >= 0.0f ? v : 0.2f * v;
    case SNTC_EPI_DEQUANT: return v + (float)reinterpret_cast<const int*>(res)[idx];
    default: return v;
  }
}

// workgroups per CU the register budget must allow (= waves per SIMD for 256-thread workgroups): what the LDS ring admits
constexpr int gg_waves(int tiles) { return tiles == 1 ? 4 : (tiles <= 3 ? 3 : 2); }

// instances of the register-staged vector pipeline whose K loop runs with compile-time ring slots (SLOTS3 in gg_kernel; the
// library-wide switch is kGGRingSlots, sntc_internal.h).  An instance is listed only if the loop keeps its waves per SIMD and adds
// no spill (tools/kernel_resources.py): every shape but 256 x 128, which sits at 255 registers with the old loop
// and spills two with the new one
constexpr bool gg_const_slots(int TM, int TN) { return !(TM == 2 && TN == 4); }

// BF3 (experiment, DESIGN.md 8: "bf16 x 3"): every fp32 operand is split into three bfloat16 terms hi + mid + lo (24
// mantissa bits together) and the product is accumulated in fp32 from the six significant cross terms on
// v_mfma_f32_32x32x16_bf16 -- 6 MFMAs of 32 cycles for K = 16 against 8 fp32 MFMAs of 64 cycles.  The weights are split
// once at pack time, the activations while they are staged into LDS.  Results are NOT bit-identical to the fp32 path
// (the dropped terms are ~2^-24 relative, and the summation order inside an MFMA differs): a fenced decode experiment.
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ void split3(float x, __bf16* hi, __bf16* mid, __bf16* lo) {
  const __bf16 h = (__bf16)x;
  const float r1 = x - (float)h;               // exact
  const __bf16 m = (__bf16)r1;
  const float r2 = r1 - (float)m;              // exact
  *hi = h; *mid = m; *lo = (__bf16)r2;
}

// DMA: the stage tiles go from L2 / HBM straight into the LDS ring (buffer_load ... lds): no staging registers, no
// ds_write, and the data never crosses the vector register file.  The LDS destination of a wave instruction is linear
// (64 lanes x 16 B = 16 rows), so the XOR swizzle is applied to the SOURCE chunk each lane fetches.  Four ring slots: stage
// j+3 is issued in step j, stage j+2 is waited for (counted vmcnt) before the barrier of step j, and its first fragments are
// prefetched in step j+1.
template <int TM, int TN, int WM, int WN, bool VEC, bool PRO, bool BF3 = false, bool DMA = false, int DEEP = 0, bool FUSE2 = false,
          bool COLM = false>
__global__ void __launch_bounds__(256, FUSE2 ? 2 : gg_waves(TM * TN)) gg_kernel(const GGArgs a) {
  static_assert(!BF3 || (VEC && !PRO), "the bf16 x 3 experiment covers the vector path without prologue");
  static_assert(!DMA || (VEC && !PRO && !BF3), "direct-to-LDS staging: vector path, no prologue (nothing can touch the data on the way)");
  static_assert(!FUSE2 || (TM == 1 && TN == 3 && WM == 4 && WN == 1 && VEC && !PRO && !BF3 && !DMA),
                "FUSE2: 3x3 (N = 96) -> 1x1 (96 -> 192) of a ResidualBlock, the 128 x 96 register-staged instance only");
  static_assert(DEEP == 0 || (DMA && (DEEP & (DEEP - 1)) == 0 && DEEP >= 4), "DEEP: ring slots of the direct-to-LDS pipeline, a power of two");
  constexpr int RING = DMA ? (DEEP ? DEEP : 4) : 3;
  constexpr int BM = WM * TM * 32;
  constexpr int BN = WN * TN * 32;
  // floats per ring slot.  fp32: A rows, then B rows, 16 floats (64 B) each.  BF3: three bf16 planes of A rows, then three of
  // B rows, 16 bf16 (32 B) per row and plane = 96 B per row
  constexpr int SLOT = BF3 ? (BM + BN) * 24 : (BM + BN) * kStage;
  constexpr int A_CH = BM / 64;                       // 16-B chunks per thread per stage (A, vector path)
  constexpr int B_CH = BF3 ? (BN * 6 + 255) / 256 : (BN + 63) / 64;   // BF3: 6 chunks of 16 B per weight row and stage
  constexpr int A_SC = BM / 16;                       // dwords per thread per stage (A, gather path)
  constexpr int EPW = 32 * (TN >= 2 ? 64 : 32);       // floats of epilogue staging per wave
  constexpr bool DBUF = !BF3 && TM * TN <= 8 && TN <= 5;   // fragment double buffering (the two widest 32-row tiles, 96+ accumulator
                                                      // registers and 7-8 fragment quads, run single-buffered)
  // TWO: two staging register sets alternate through the whole K loop (stage s lives in set s & 1): the global loads of stage
  // j+4 are issued in step j into the set step j has just written to LDS, two steps before step j+2 writes them -- twice the
  // lead of the single set, for no LDS.  OFF in the shipped library (kGGTwoSets, sntc_internal.h): it measured 4 - 6 % SLOWER
  // on the hyper-synthesis launches, with the same bits.  Compiled only where the second set fits the instance's
  // waves per SIMD without a spill: the one- and two-tile instances (128 x 64: 167 of 168 registers) and the 2 x 2-tile
  // 128 x 128 one with its column-major twin; 128 x 96 sits at 163 of 168 registers, the 1 x 4-tile 128 x 128 instance spills
  // 71 registers with a second set and the wider tiles have no room: they keep the single set either way
  constexpr bool TWO = kGGTwoSets && VEC && DBUF && !DMA && !FUSE2 && (TM * TN <= 2 || (TM == 2 && TN == 2));
  // SLOTS3: the single-set loop runs three stages per iteration with the ring slots 0, 1, 2 as compile-time constants (every piece
  // starts at slot 0, so stage j of a piece sits in slot j % 3): the LDS addresses of write_lds / read_frag are a loop-invariant
  // lane register plus an immediate instead of slot * SLOT + lane offset re-made every stage, and the rotation of three slot
  // registers goes.  Per instance (gg_const_slots): only where the register count holds the instance's waves per SIMD without a spill
  // (the prologue instances keep the old loop as well: with abs / square between the staging registers and LDS the compiler
  // rejects the walk's scalar pin in advance_stage)
  constexpr bool SLOTS3 = kGGRingSlots && VEC && !PRO && !BF3 && !DMA && !TWO && gg_const_slots(TM, TN);
  constexpr bool RBUF = TWO || (DBUF && TM * TN <= 3 && !FUSE2);   // second staging register set for a tile's first two stages
  static_assert(RING * SLOT >= 4 * EPW + (DMA ? SLOT : 0), "epilogue staging (and one prefetched stage) must fit in the stage ring");
  if constexpr (SLOTS3 && !COLM) {
    // register floor: the loop needs a few registers fewer than the old one, which takes 128 x 64 (129 -> 127) and the strip-major
    // 128 x 128 (169 -> 166) under an occupancy edge: the hardware could then hold one workgroup more of them on a CU than the
    // instance's __launch_bounds__ and the schedules measured with it count on.  With the worker counts held where they were,
    // that build ran the two-stream step 1.3 % slower, the 18-image HS2 stream-K launch 500 or 630 us from step to step
    // (DESIGN.md 8).  Naming the first register past the edge of W + 1 waves per SIMD (512 registers, allocated in eights)
    // keeps the allocation at the launch bound's W.  The column-major twin has none: it is the one instance that runs above
    // its launch bound on purpose (three per CU at 166 <= 168 registers)
    constexpr int W = FUSE2 ? 2 : gg_waves(TM * TN);
    if constexpr (W == 2) asm volatile("" ::: "v168");        // 169 registers -> 176 allocated: two waves
    else if constexpr (W == 3) asm volatile("" ::: "v128");   // 129 -> 136: three
    else asm volatile("" ::: "v96");                          // 97 -> 104: four
  }
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* ring = reinterpret_cast<float*>(smem);                  // [RING][BM + BN][16]
  int4* rinfo_all = reinterpret_cast<int4*>(ring + RING * SLOT); // [2][BM] (n, qy, qx, valid) of the current / next tile

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wm = wave / WN;
  const int wn = wave % WN;
  const int l31 = lane & 31;
  const int h = lane >> 5;

  // ------------------------------------------------------------------------------------------------------
  // the worker's list of pieces
  // ------------------------------------------------------------------------------------------------------
  // stream-K: the walk over this worker's share (gg_pieces.h; COLM: the column-major unit order, at compile time); static: one piece
  PieceWalk<COLM ? kOrderColumn : kOrderStrip> walk;
  Piece P;
  if (a.sk) {
    walk.init(a, blockIdx.x);
    if (!walk.next(fresh_args(), &P)) return;
  } else {
    static_piece(a, blockIdx.x, &P);
  }

  // ------------------------------------------------------------------------------------------------------
  // per-piece loader state
  // ------------------------------------------------------------------------------------------------------
  const __amdgpu_buffer_rsrc_t xs =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.x), 0, (int)a.x_bytes, 0x00020000);
  const int r0 = tid >> 2;        // vector path: row 0..63 (+64 i)
  // vector path: 16-B chunk inside the 64-B K slab this lane fetches.  Register staging: lane (tid & 3) fetches chunk
  // tid & 3 and WRITES it to the swizzled LDS position; DMA: the LDS position is the lane's own (linear destination), so
  // the lane fetches the chunk that belongs there
  const int c = DMA ? ((tid & 3) ^ ((r0 >> 2) & 3)) : (tid & 3);
  const int wsw = (c ^ ((r0 >> 2) & 3)) << 2;
  const int kk = tid & 15;        // gather path: k column inside the stage
  const int rs = tid >> 4;        // gather path: row 0..15 (+16 i)
  const int gsw = (((kk >> 2) ^ ((rs >> 2) & 3)) << 2) + (kk & 3);
  constexpr int NROW = VEC ? A_CH : A_SC;

  int a_iy0[NROW], a_ix0[NROW];
  unsigned a_img[NROW];           // byte offset of the row's image (+ chunk), or kOutOfRange for padding rows
  unsigned a_off[NROW];           // vector path: current tap's byte offset per row
  // vector path (kGGTapState): per-tile row state of gg_tap_rules.h -- byte offset of tap (0, 0) mod 2^32, and the taps whose
  // image row (bits 0..15) / column (bits 16..31) is inside the image -- so that a tap change costs an add and a mask test
  unsigned a_base[NROW], a_mask[NROW];
  unsigned ld_delta = 0, ld_sel = 0x10001u;     // wave-uniform: the current tap's byte delta against tap (0, 0), its select word
  unsigned tap_dx = 0, tap_drow = 0;            // delta steps: next tap in the row; first tap of the next row
  unsigned b_off[B_CH];
  int ld_stage = 0, ld_t = 0, ld_cc = 0;        // next stage to load; vector path: its (tap, channel slab)
  int ld_ty = 0, ld_tx = 0;                     // vector path: the tap's (row, column) in the group's tw-wide tap grid
  int g_t = 0, g_ch = 0, g_ty = 0, g_tx = 0;    // gather path: (tap, channel) of this thread's k column
  int g_T = a.g[P.gi].T, g_tw = a.g[P.gi].tw;   // hot fields of the current piece's group: taps form a dense grid, tap t
                                                // = (t / tw, t % tw), walked incrementally (no table load in the loop)
  __amdgpu_buffer_rsrc_t ws =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.g[P.gi].wp), 0, a.g[P.gi].Ncol * a.g[P.gi].K * (BF3 ? 6 : 4), 0x00020000);
  int m0 = 0, n0 = 0;

  auto set_tap = [&](int ty, int tx) {
    if constexpr (kGGTapState) {
#pragma unroll
      for (int i = 0; i < NROW; ++i) a_off[i] = gg_tap_offset(a_base[i], a_mask[i], ld_delta, ld_sel);
      return;
    }
#pragma unroll
    for (int i = 0; i < NROW; ++i) {
      const int iy = a_iy0[i] + ty * a.tstep;
      const int ix = a_ix0[i] + tx * a.tstep;
      const bool ok = (unsigned)iy < (unsigned)a.H && (unsigned)ix < (unsigned)a.W;
      const unsigned pix = ((unsigned)(iy * a.W + ix) * (unsigned)a.Cin * 4u) & 0x7fffffffu;
      // branch-free: in-range sums stay below 2^31 (host check); a padding row (a_img = 2^31) or a tap outside the image
      // gets bit 31 and reads zeros from the descriptor's bounds check
      a_off[i] = (a_img[i] + pix) | (ok ? 0u : kOutOfRange);
    }
  };

  auto init_loader = [&](const Piece& p, int rb) {
    KArgs& a = fresh_args();
    const int4* rinfo = rinfo_all + rb * BM;
    const auto& G = a.g[p.gi];
    g_T = G.T;
    g_tw = G.tw;
    ws = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(G.wp), 0, G.Ncol * G.K * (BF3 ? 6 : 4), 0x00020000);
    m0 = p.mt * BM;
    n0 = p.nt * BN;
#pragma unroll
    for (int i = 0; i < NROW; ++i) {
      const int4 ri = rinfo[VEC ? r0 + 64 * i : rs + 16 * i];
      if constexpr (VEC && kGGTapState) {
        const TapGeo geo{a.H, a.W, a.Cin, a.sA, a.tstep, a.offy, a.offx};
        gg_tap_row(geo, ri.x, ri.y, ri.z, ri.w, c, g_T / g_tw, g_tw, &a_base[i], &a_mask[i]);
        continue;
      }
      a_iy0[i] = ri.y * a.sA + a.offy;
      a_ix0[i] = ri.z * a.sA + a.offx;
      a_img[i] = ri.w ? (unsigned)ri.x * (unsigned)(a.H * a.W) * (unsigned)a.Cin * 4u + (VEC ? (unsigned)c * 16u : 0u)
                      : kOutOfRange;
    }
#pragma unroll
    for (int i = 0; i < B_CH; ++i) {   // rows past Ncol re-read the last column (finite, discarded)
      if (BF3) {                        // chunk q of the tile's stage: weight row q / 6, 16-B part q % 6 = (plane, half)
        const int q = tid + 256 * i;
        const int brow = min(n0 + q / 6, G.Ncol - 1);
        b_off[i] = (unsigned)brow * (unsigned)(G.K / kStage) * 96u + (unsigned)(q % 6) * 16u;
      } else {
        const int brow = min(n0 + r0 + 64 * i, G.Ncol - 1);
        b_off[i] = (unsigned)brow * (unsigned)G.K * 4u + (unsigned)c * 16u;
      }
    }
    ld_stage = p.k0;
    if (VEC) {
      ld_cc = p.k0 / g_T;
      ld_t = p.k0 - ld_cc * g_T;
      ld_ty = ld_t / g_tw;
      ld_tx = ld_t - ld_ty * g_tw;
      if constexpr (kGGTapState) {
        const TapGeo geo{a.H, a.W, a.Cin, a.sA, a.tstep, a.offy, a.offx};
        tap_dx = gg_tap_dx(geo);
        tap_drow = gg_tap_dy(geo) - (unsigned)(g_tw - 1) * tap_dx;
        ld_delta = gg_tap_delta(geo, ld_ty, ld_tx);
        ld_sel = gg_tap_select(ld_ty, ld_tx);
      }
      set_tap(ld_ty, ld_tx);
    } else {
      const int k = p.k0 * kStage + kk;
      g_t = k / a.Cin;
      g_ch = k - g_t * a.Cin;
      g_ty = g_t / g_tw;
      g_tx = g_t - g_ty * g_tw;
    }
  };

  struct Regs {
    f32x4 a[VEC ? A_CH : 1];
    float s[VEC ? 1 : A_SC];
    f32x4 b[B_CH];
  };

  auto advance_stage = [&]() {
    ++ld_stage;
    if (VEC) {
      // next stage's channel slab / tap, without a branch (the steady-state loop stays one basic block: the scheduler
      // can then place every load, LDS write and fragment read between MFMAs); the per-row offsets are re-made every
      // stage from the row's (base, mask) and the scalar (delta, select) -- 4 VALU per row (kGGTapState off: the whole
      // source-pixel formula, ~10 VALU per row with two quarter-rate multiplies)
      // K order of the vector path: channel slab OUTERMOST, taps inside (k = cc * T * 16 + t * 16 + c): the taps of one
      // 16-channel slab re-read the same input pixels (a 5x5 / stride-2 layer touches each ~6 times), so they now do it
      // within T consecutive stages, from L2, instead of T * Cin / 16 stages apart, from HBM
      const int row_end = (ld_tx + 1 == g_tw) ? 1 : 0;
      const int tap_end = (ld_t + 1 == g_T) ? 1 : 0;
      ld_tx = row_end ? 0 : ld_tx + 1;
      ld_ty = tap_end ? 0 : ld_ty + row_end;
      ld_t = tap_end ? 0 : ld_t + 1;
      ld_cc += tap_end;
      if constexpr (kGGTapState) {          // scalar: the delta walks the tap grid with adds, and starts over at the slab's end
        ld_delta = tap_end ? 0u : ld_delta + (row_end ? tap_drow : tap_dx);
        ld_sel = gg_tap_select(ld_ty, ld_tx);
      }
      if constexpr (SLOTS3) {
        // the walk's state stays in scalar registers from one step to the next: with three steps in one loop body the compiler
        // otherwise merges their tap_end chains, carries the flags in vector registers (ld_cc += tap_end becomes v_addc_co), and
        // every buffer load gets a waterfall loop for its now "divergent" scalar offset
        asm volatile("" : "+s"(ld_cc), "+s"(ld_t), "+s"(ld_ty), "+s"(ld_tx));
        if constexpr (kGGTapState) asm volatile("" : "+s"(ld_delta), "+s"(ld_sel));
      }
      set_tap(ld_ty, ld_tx);
    }
  };

  auto load_regs = [&](Regs& R) {
    if (VEC) {
      const unsigned soff = (unsigned)ld_cc * 64u;
#pragma unroll
      for (int i = 0; i < A_CH; ++i) R.a[i] = buf_load(xs, a_off[i], soff);
    } else {
      const bool kok = g_t < g_T;
      const int ty = g_ty * a.tstep, tx = g_tx * a.tstep;
#pragma unroll
      for (int i = 0; i < A_SC; ++i) {
        const int iy = a_iy0[i] + ty;
        const int ix = a_ix0[i] + tx;
        const bool ok = kok && (unsigned)iy < (unsigned)a.H && (unsigned)ix < (unsigned)a.W && !(a_img[i] & kOutOfRange);
        const unsigned off = a_img[i] + ((unsigned)(iy * a.W + ix) * (unsigned)a.Cin + (unsigned)g_ch) * 4u;
        R.s[i] = buf_load1(xs, ok ? off : kOutOfRange);
      }
      g_ch += kStage;
      while (g_ch >= a.Cin) {
        g_ch -= a.Cin;
        ++g_t;
        if (++g_tx == g_tw) { g_tx = 0; ++g_ty; }
      }
    }
    const unsigned wsoff = (unsigned)ld_stage * (BF3 ? 96u : 64u);
#pragma unroll
    for (int i = 0; i < B_CH; ++i)
      if (BF3 ? ((BN * 6) % 256 == 0 || tid + 256 * i < BN * 6) : (BN % 64 == 0 || r0 + 64 * i < BN))
        R.b[i] = buf_load(ws, b_off[i], wsoff);
    advance_stage();
  };

  // DMA: this wave's share of one stage, HBM / L2 -> LDS slot.  Instruction i of wave w lands on rows 16 w + 64 i ... + 15
  // (64 lanes x 16 B, linear); the per-lane source offsets are the register path's (with the source-side swizzle in c)
  const int my_nb = [&]() {                    // B instructions this wave issues per stage (rows 16 w + 64 i < BN)
    int nb = 0;
#pragma unroll
    for (int i = 0; i < B_CH; ++i) nb += ((tid >> 6) * 16 + 64 * i < BN) ? 1 : 0;
    return nb;
  }();
  const int wave_u = __builtin_amdgcn_readfirstlane(tid >> 6);      // provably wave-uniform: the LDS destination (M0) and the
                                                                    // scalar offsets must not make the compiler build waterfall loops
  auto dma_stage = [&](int slot) {
    typedef __attribute__((address_space(3))) void lds_void;
    float* Ab = ring + __builtin_amdgcn_readfirstlane(slot) * SLOT + wave_u * 16 * kStage;
    const unsigned soff = (unsigned)__builtin_amdgcn_readfirstlane(ld_cc) * 64u;
#pragma unroll
    for (int i = 0; i < A_CH; ++i)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(xs, (lds_void*)(Ab + 64 * i * kStage), 16, (int)a_off[i], (int)soff, 0, 0);
    float* Bb = Ab + BM * kStage;
    const unsigned wsoff = (unsigned)__builtin_amdgcn_readfirstlane(ld_stage) * 64u;
#pragma unroll
    for (int i = 0; i < B_CH; ++i)
      if (BN % 64 == 0 || wave_u * 16 + 64 * i < BN)
        __builtin_amdgcn_raw_ptr_buffer_load_lds(ws, (lds_void*)(Bb + 64 * i * kStage), 16, (int)b_off[i], (int)wsoff, 0, 0);
    advance_stage();
  };
  // wait until at most K of this wave's DMA stages are outstanding (vmcnt counts instructions, in order); K is a compile-time
  // constant because s_waitcnt takes an immediate
  auto dma_wait = [&](auto K) {
    constexpr int k = decltype(K)::value < 0 ? 0 : decltype(K)::value;
    if (k == 0) {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    } else if (my_nb == B_CH) {
      asm volatile("s_waitcnt vmcnt(%0)" ::"n"(k * (A_CH + B_CH)) : "memory");
    } else {
      asm volatile("s_waitcnt vmcnt(%0)" ::"n"(k * (A_CH + B_CH - 1)) : "memory");
    }
  };
  auto write_lds = [&](const Regs& R, int slot) {
    float* Ab = ring + slot * SLOT;
    if (BF3) {
      // A: split the four fp32 values of this thread's chunk into three bf16 quads; plane p of row r lives at
      // p * BM * 32 + r * 32 bytes, its two 16-B halves swapped by (r >> 3) & 1 (conflict-free fragment reads)
      char* Ap = reinterpret_cast<char*>(Ab);
      char* Bp = Ap + 3 * BM * 32;
#pragma unroll
      for (int i = 0; i < A_CH; ++i) {
        const int r = r0 + 64 * i;
        bf16x4 hi, mid, lo;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          __bf16 x0, x1, x2;
          split3(R.a[i][e], &x0, &x1, &x2);
          hi[e] = x0; mid[e] = x1; lo[e] = x2;
        }
        const int off = r * 32 + (((c >> 1) ^ ((r >> 3) & 1)) << 4) + ((c & 1) << 3);
        *reinterpret_cast<bf16x4*>(Ap + off) = hi;
        *reinterpret_cast<bf16x4*>(Ap + BM * 32 + off) = mid;
        *reinterpret_cast<bf16x4*>(Ap + 2 * BM * 32 + off) = lo;
      }
#pragma unroll
      for (int i = 0; i < B_CH; ++i) {
        const int q = tid + 256 * i;
        if ((BN * 6) % 256 == 0 || q < BN * 6) {
          const int r = q / 6, part = q % 6, plane = part >> 1, half = part & 1;
          *reinterpret_cast<f32x4*>(Bp + plane * BN * 32 + r * 32 + ((half ^ ((r >> 3) & 1)) << 4)) = R.b[i];
        }
      }
      return;
    }
    float* Bb = Ab + BM * kStage;
    if (VEC) {
#pragma unroll
      for (int i = 0; i < A_CH; ++i) {
        f32x4 v = R.a[i];
        if (PRO) {
          if (a.pro == SNTC_PRO_ABS) {
            v[0] = fabsf(v[0]); v[1] = fabsf(v[1]); v[2] = fabsf(v[2]); v[3] = fabsf(v[3]);
          } else if (a.pro == SNTC_PRO_SQUARE) {
            v = v * v;
          }
        }
        *reinterpret_cast<f32x4*>(Ab + (r0 + 64 * i) * kStage + wsw) = v;
      }
    } else {
#pragma unroll
      for (int i = 0; i < A_SC; ++i) {
        float v = R.s[i];
        if (PRO) {
          if (a.pro == SNTC_PRO_ABS) v = fabsf(v);
          else if (a.pro == SNTC_PRO_SQUARE) v = v * v;
        }
        Ab[(rs + 16 * i) * kStage + gsw] = v;
      }
    }
#pragma unroll
    for (int i = 0; i < B_CH; ++i)
      if (BN % 64 == 0 || r0 + 64 * i < BN)
        *reinterpret_cast<f32x4*>(Bb + (r0 + 64 * i) * kStage + wsw) = R.b[i];
  };

  // fragment addresses: row = 32-row block + l31, chunk (2g + h) ^ ((row >> 2) & 3)
  const int swz = (l31 >> 2) & 3;
  const int fa_row = (wm * TM * 32 + l31) * kStage;
  const int fb_row = (BM + wn * TN * 32 + l31) * kStage;
  const int foff0 = ((0 + h) ^ swz) << 2, foff1 = ((2 + h) ^ swz) << 2;

  struct Frag {
    f32x4 a[TM];
    f32x4 b[TN];
  };
  auto read_frag = [&](Frag& F, int slot, int g) {
    const float* base = ring + slot * SLOT;
    const int off = g ? foff1 : foff0;
#pragma unroll
    for (int i = 0; i < TM; ++i) F.a[i] = *reinterpret_cast<const f32x4*>(base + fa_row + i * 32 * kStage + off);
#pragma unroll
    for (int j = 0; j < TN; ++j) F.b[j] = *reinterpret_cast<const f32x4*>(base + fb_row + j * 32 * kStage + off);
  };

  struct Frag3 {
    bf16x8 a[BF3 ? 3 : 1][TM];
    bf16x8 b[BF3 ? 3 : 1][TN];
  };
  auto read_frag3 = [&](Frag3& F, int slot) {
    const char* base = reinterpret_cast<const char*>(ring + slot * SLOT);
    const int hoff = (h ^ ((l31 >> 3) & 1)) << 4;
#pragma unroll
    for (int p = 0; p < (BF3 ? 3 : 1); ++p) {
#pragma unroll
      for (int i = 0; i < TM; ++i)
        F.a[p][i] = *reinterpret_cast<const bf16x8*>(base + p * BM * 32 + (wm * TM * 32 + i * 32 + l31) * 32 + hoff);
#pragma unroll
      for (int j = 0; j < TN; ++j)
        F.b[p][j] = *reinterpret_cast<const bf16x8*>(base + 3 * BM * 32 + p * BN * 32 + (wn * TN * 32 + j * 32 + l31) * 32 + hoff);
    }
  };

  f32x16 acc[TM][TN];
  auto mfma3 = [&](const Frag3& F) {           // smallest terms first: lo*hi, hi*lo, mid*mid, mid*hi, hi*mid, hi*hi
    constexpr int PA[6] = {2, 0, 1, 1, 0, 0};
    constexpr int PB[6] = {0, 2, 1, 0, 1, 0};
#pragma unroll
    for (int t = 0; t < (BF3 ? 6 : 0); ++t)
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(F.a[BF3 ? PA[t] : 0][i], F.b[BF3 ? PB[t] : 0][j], acc[i][j], 0, 0, 0);
  };
  auto mfma_group = [&](const Frag& F) {
    if (SNTC_DBG(a, 64)) return;
#pragma unroll
    for (int e = 0; e < 4; ++e)
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
          acc[i][j] = FUSE2 ? __builtin_amdgcn_mfma_f32_32x32x2f32(F.b[j][e], F.a[i][e], acc[i][j], 0, 0, 0)
                            : __builtin_amdgcn_mfma_f32_32x32x2f32(F.a[i][e], F.b[j][e], acc[i][j], 0, 0, 0);
  };

  // ------------------------------------------------------------------------------------------------------
  // the piece loop
  // ------------------------------------------------------------------------------------------------------
  int rb = 0;                                  // rinfo buffer of the current piece
  Regs R0, R1;
  write_rinfo<BM, 256>(fresh_args(), P, rinfo_all + rb * BM, tid);
  __syncthreads();
  init_loader(P, rb);
  int dma_issued = 0;                          // DMA: stages of the current piece already on their way (slots 0 ...)
  if (DMA) {
    const int n = P.k1 - P.k0;
    for (; dma_issued < RING - 1 && dma_issued < n; ++dma_issued) dma_stage(dma_issued);
  } else {
    const int n = P.k1 - P.k0;
    if (n > 0) load_regs(R0);
    if (RBUF && n > 1) load_regs(R1);
  }

  while (true) {
    const int n = P.k1 - P.k0;
    // ---- accumulators: zero, or the previous worker's published partial sums (stream-K continuation)
    if (P.consume >= 0) {
      sk_consume<TM, TN, 256>(a, P.consume, tid, acc);
    } else {
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
          for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.0f;
    }

    Frag F0, F1;
    if (DMA) {
      // ---- direct-to-LDS pipeline: stages 0 .. RING-2 are (being) issued; slot of stage j is j & (RING-1).  Step j issues
      // stage j + RING - 1 into the slot stage j - 1 left at the last barrier and ends once stage j + 2 has landed, so
      // RING - 3 younger stages stay in flight across the barrier (1 with the 4-slot ring; 5 with the 8-slot ring of
      // the DEEP instances, which launches too small to hide the memory latency behind other workgroups are given)
      for (; dma_issued < RING - 1 && dma_issued < n; ++dma_issued) dma_stage(dma_issued);
      // stages 0 and 1 must have landed before the first step (stage 1's fragments are prefetched in step 0)
      using Yes = std::integral_constant<bool, true>;
      using No = std::integral_constant<bool, false>;
      auto wait_first = [&](auto I) {           // issued = min(n, RING - 1) stages; all but the first two may still fly
        constexpr int i = decltype(I)::value;
        if constexpr (i > 2) {
          if (n >= i) { dma_wait(std::integral_constant<int, i - 2>{}); return true; }
        }
        return false;
      };
      if (!first_of_desc<RING - 1, 3>(wait_first)) dma_wait(std::integral_constant<int, 0>{});
      __builtin_amdgcn_s_barrier();
      __builtin_amdgcn_sched_barrier(0);
      if (n > 0) read_frag(F0, 0, 0);
      // REM: steps left including this one when no stage is left to issue (compile-time, for the counted wait); -1 in the
      // steady state
      auto dstep = [&](int j, auto LD, auto PF, auto REM) {
        if (decltype(LD)::value) dma_stage((j + RING - 1) & (RING - 1));   // slot of stage j - 1, free since the last barrier
        read_frag(F1, j & (RING - 1), 1);
        mfma_group(F0);
        if (decltype(PF)::value) read_frag(F0, (j + 1) & (RING - 1), 0);
        mfma_group(F1);
        if (decltype(LD)::value) {
          constexpr int NW = A_CH + B_CH, NR = TM + TN, NM = 4 * TM * TN;
          __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
          __builtin_amdgcn_sched_group_barrier(0x020, NW, 0);
          __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
          __builtin_amdgcn_sched_group_barrier(0x100, NR, 0);
          __builtin_amdgcn_sched_group_barrier(0x008, NM - 2, 0);
          __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
          __builtin_amdgcn_sched_group_barrier(0x100, NR, 0);
          __builtin_amdgcn_sched_group_barrier(0x008, NM - 1, 0);
        }
        __builtin_amdgcn_sched_barrier(0);
        // stage j + 2 has landed; the younger ones may still fly
        if constexpr (decltype(LD)::value) dma_wait(std::integral_constant<int, RING - 3>{});
        else dma_wait(std::integral_constant<int, decltype(REM)::value - 3>{});
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_sched_barrier(0);
      };
      int j = 0;
      for (; j + RING - 1 < n; ++j) dstep(j, Yes{}, Yes{}, std::integral_constant<int, -1>{});
      // the last RING - 1 (or fewer) steps: everything is issued, the counted wait shrinks with the steps left
      auto tail = [&](auto REM) {
        constexpr int rem = decltype(REM)::value;
        if (n - j == rem) {
          if constexpr (rem > 1) dstep(j, No{}, Yes{}, REM);
          else dstep(j, No{}, No{}, REM);
          ++j;
        }
      };
      first_of_desc<RING - 1, 1>([&](auto REM) { tail(REM); return false; });
      dma_issued = 0;
    } else {
    // ---- prologue: stages k0, k0+1 -> ring slots 0, 1; stage k0+2 in flight
    int r_cur = 0, r_n1 = 1, r_n2 = 2;
    if (n > 0) write_lds(R0, 0);
    if (RBUF) {
      if (n > 1) write_lds(R1, 1);
    } else if (n > 1) {
      load_regs(R0);
      write_lds(R0, 1);
    }
    if (n > 2) load_regs(R0);
    if (TWO && n > 3) load_regs(R1);           // two sets: stages k0+2 and k0+3 in flight
    __syncthreads();
    if (DBUF && n > 0) read_frag(F0, 0, 0);

    // one step = one stage.  WR: stage j+2 goes from registers into the ring; LD: stage j+3's global loads are issued;
    // PF: the first fragments of stage j+1 are prefetched.  The steady-state steps have all three and no branch.
    // R: the staging set of the step (single set: always R0; TWO: the set of the step's parity, stage j+2 loaded during step
    // j-2, stage j+4 issued now)
    // S: the ring slot of stage j as a compile-time constant (SLOTS3), or -1: the slots are the rotating s_cur / s_n1 / s_n2
    auto step = [&](Regs& R, auto WR, auto LD, auto PF, auto S) {
      constexpr int kS = decltype(S)::value;
      const int s_cur = kS < 0 ? r_cur : kS, s_n1 = kS < 0 ? r_n1 : (kS + 1) % 3, s_n2 = kS < 0 ? r_n2 : (kS + 2) % 3;
      if (gg_flag(WR) && !SNTC_DBG(a, 2)) write_lds(R, s_n2);                 // stage j+2, loaded during step j-1 (TWO: j-2)
      if (gg_flag(LD) && !SNTC_DBG(a, 1)) load_regs(R);                       // stage j+3 (TWO: j+4)
      if (BF3) {
        Frag3 F3;
        read_frag3(F3, s_cur);
        mfma3(F3);
      } else if (DBUF) {
        if (!SNTC_DBG(a, 8)) read_frag(F1, s_cur, 1);
        mfma_group(F0);
        if (gg_flag(PF) && !SNTC_DBG(a, 8)) read_frag(F0, s_n1, 0);           // under this stage's remaining MFMAs
        mfma_group(F1);
      } else {
        read_frag(F0, s_cur, 0);
        mfma_group(F0);
        read_frag(F0, s_cur, 1);
        mfma_group(F0);
      }
      if constexpr (DBUF && VEC && gg_yes<decltype(WR)> && gg_yes<decltype(LD)> && gg_yes<decltype(PF)>) {
        // steady state: order the step's memory instructions BETWEEN its MFMAs (mask 0x8 MFMA, 0x200 DS write, 0x20 VMEM
        // read, 0x100 DS read): an MFMA occupies the pipe for 64 cycles but its issue slot for a few, so everything
        // placed behind the first one is free; the fragment reads get a full MFMA group to land before they are used
        constexpr int NW = A_CH + B_CH, NR = TM + TN, NM = 4 * TM * TN;
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x200, NW, 0);
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x020, NW, 0);
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x100, NR, 0);
        __builtin_amdgcn_sched_group_barrier(0x008, NM - 3, 0);
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x100, NR, 0);
        __builtin_amdgcn_sched_group_barrier(0x008, NM - 1, 0);
      }
      __builtin_amdgcn_sched_barrier(0);                   // every MFMA of the step is issued before the wave waits
      if (!SNTC_DBG(a, 4)) __syncthreads();
      __builtin_amdgcn_sched_barrier(0);
      if constexpr (kS < 0) { r_cur = s_n1; r_n1 = s_n2; r_n2 = s_cur; }
    };
    using Yes = std::integral_constant<bool, true>;
    using No = std::integral_constant<bool, false>;
    using Rot = std::integral_constant<int, -1>;
    if constexpr (TWO) {
      // steady state: two steps per iteration, R0 on the even and R1 on the odd stages of the piece, no register copies.  ONE
      // exit, after a whole pair (a second exit between the two steps made the compiler carry the accumulators out of the loop
      // in a second register set: 16 to 32 v_mov_b64 per iteration); a fifth remaining step is the pair's first half again
      int j = 0;
      for (; j + 5 < n; j += 2) {
        step(R0, Yes{}, Yes{}, Yes{}, Rot{});
        step(R1, Yes{}, Yes{}, Yes{}, Rot{});
      }
      int rem = n - j;                         // 0 .. 5
      bool odd = false;
      if (rem == 5) {
        step(R0, Yes{}, Yes{}, Yes{}, Rot{});
        odd = true;
        rem = 4;
      }
      // tail: up to two stages wait in the sets (stage j+2 in the set of j's parity, then stage j+3 in the other)
      if (rem >= 4) {
        if (odd) step(R1, Yes{}, No{}, Yes{}, Rot{}); else step(R0, Yes{}, No{}, Yes{}, Rot{});
        odd = !odd;
      }
      if (rem >= 3) {
        if (odd) step(R1, Yes{}, No{}, Yes{}, Rot{}); else step(R0, Yes{}, No{}, Yes{}, Rot{});
      }
      if (rem >= 2) step(R0, No{}, No{}, Yes{}, Rot{});
      if (rem >= 1) step(R0, No{}, No{}, No{}, Rot{});
    } else if constexpr (SLOTS3) {
      // steady state: three steps per iteration, stage j in slot j % 3.  ONE exit, after a whole triple (see TWO above).  The
      // 0 .. 5 steps left: one copy per POSITION (its slot a constant), what the step still writes, loads and prefetches a
      // run-time flag of the steps left.  One straight line per remainder was tried first: the compiler then keeps the
      // accumulators in two register sets across the five-way branch (+32 registers on 128 x 64, +64 on 128 x 128)
      int j = 0;
#pragma unroll 1
      for (; j + 5 < n; j += 3) {
        step(R0, Yes{}, Yes{}, Yes{}, std::integral_constant<int, 0>{});
        step(R0, Yes{}, Yes{}, Yes{}, std::integral_constant<int, 1>{});
        step(R0, Yes{}, Yes{}, Yes{}, std::integral_constant<int, 2>{});
      }
      const int rem = n - j;
      each_of<5>([&](auto Pc) {
        const int left = rem - decltype(Pc)::value;                            // steps left, this one included
        if (left > 0) step(R0, left >= 3, left > 3, left >= 2, std::integral_constant<int, decltype(Pc)::value % 3>{});
      });
    } else {
      for (int j = 0; j + 3 < n; ++j) step(R0, Yes{}, Yes{}, Yes{}, Rot{});
      if (n >= 3) step(R0, Yes{}, No{}, Yes{}, Rot{});
      if (n >= 2) step(R0, No{}, No{}, Yes{}, Rot{});
      if (n >= 1) step(R0, No{}, No{}, No{}, Rot{});
    }
    }   // register-staged pipeline

    // ---- the next piece's first stages go in flight before this piece's results are stored
    Piece Q;
    const bool more = walk.next(fresh_args(), &Q);
    const int qb = rb ^ 1;
    const int4* rinfo = rinfo_all + rb * BM;
    const int m0d = m0, n0d = n0;
    if (more) {
      write_rinfo<BM, 256>(fresh_args(), Q, rinfo_all + qb * BM, tid);
      __syncthreads();
      init_loader(Q, qb);
      const int nq = Q.k1 - Q.k0;
      if (DMA) {
        // the epilogue stages through the TOP of the ring; the slots below it take the next piece's first stages now
        constexpr int NPF = (RING * SLOT - 4 * EPW) / SLOT < RING - 1 ? (RING * SLOT - 4 * EPW) / SLOT : RING - 1;
        for (dma_issued = 0; dma_issued < NPF && dma_issued < nq; ++dma_issued) dma_stage(dma_issued);
      } else {
        if (nq > 0) load_regs(R0);
        if (RBUF && nq > 1) load_regs(R1);
      }
    }

    // ---- finish the piece that just ran.  Lane constants and kernel arguments of this phase are re-derived from an
    // opaque copy of the thread id / of the kernel-argument pointer: the compiler would otherwise hoist them out of the
    // persistent loop and keep ~40 registers alive through the K loop for values that are used once per tile.
    int te = tid;
    asm volatile("" : "+v"(te));
    const int lane = te & 63, wave = te >> 6, l31 = lane & 31, h = lane >> 5;
    const int wm = wave / WN, wn = wave % WN;
    KArgs& a = fresh_args();          // shadows the by-value copy inside this phase
    const auto& Gd = a.g[P.gi];
    if (P.publish) {
      sk_publish<TM, TN, 256>(a, walk.wl, tid, acc);     // the next worker finishes the tile from these accumulators
    } else if (a.ksplit > 1) {
      // split-K: raw partial sums go to slab[group][split][m][col]; gg_reduce_kernel adds the splits in a
      // fixed order and applies bias / activation / epilogue, so the result does not depend on scheduling.
      float* slab = a.slab + Gd.slab_off + (size_t)P.split * a.M * Gd.Ncol;
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        const int col = n0d + (wn * TN + j) * 32 + l31;
        if (col >= Gd.Ncol) continue;
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int m = m0d + (wm * TM + i) * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
            if (m < a.M) slab[(size_t)m * Gd.Ncol + col] = acc[i][j][r];
          }
      }
    } else if constexpr (FUSE2) {
      // ---- ResidualBlock tail in the same launch: y = res + W2 . relu(W1 * x + b1) + b2 (reference common/elic.py:41-68).
      // Phase 1 above accumulated the 3x3 convolution TRANSPOSED (weights as the MFMA's A operand): lane l holds pixel
      // l % 32 of the wave's 32 rows, register r of tile j the channel 32 j + (r & 3) + 8 (r >> 2) + 4 (l / 32) -- which
      // is exactly how a lane feeds the A operand of v_mfma_f32_32x32x2_f32 (row = l % 32, k = l / 32), in exactly the k
      // order of the stand-alone 1x1 kernel's fragments (quad 2 g + h of a 16-deep stage).  So relu(acc + b1) goes into
      // the second contraction straight from the registers: no round trip through HBM or LDS, the same fma chains.
#pragma unroll
      for (int j = 0; j < 3; ++j)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          f32x4 b1 = {0.f, 0.f, 0.f, 0.f};
          if (a.bias) b1 = *reinterpret_cast<const f32x4*>(a.bias + 32 * j + 8 * q + 4 * h);
#pragma unroll
          for (int e = 0; e < 4; ++e) acc[0][j][4 * q + e] = apply_act(acc[0][j][4 * q + e] + b1[e], a.act);
        }
      // One 32-wide column tile of the output at a time (16 accumulator registers next to the 48 that hold the A operand).
      // Its slice of W2 -- packed by the host in fragment order [Q][lane][4], 12 KB -- goes through one of two buffers in the
      // idle stage ring; the next slice and this tile's residual operand are loaded while the 48 MFMAs of the tile run, and
      // the tile leaves through a wave-private 4 KB staging slice behind the two buffers.
      float* stage = ring + 2 * 3072 + wave * 1024;
      const f32x4* w2src = reinterpret_cast<const f32x4*>(a.w2f);
      f32x4 wreg[3];
#pragma unroll
      for (int u = 0; u < 3; ++u) wreg[u] = w2src[te + 256 * u];
      const int c4 = (lane & 7) << 2;                // epilogue: 8 lanes x 16 B per row, 8 rows per pass, 4 passes
      const int rsub = lane >> 3;
      const int mrow = m0d + wave * 32 + rsub;       // + 8 p: this lane's output row in pass p
      __syncthreads();                               // the K loop's last fragment reads are done: the ring is free
#pragma unroll 1
      for (int ct = 0; ct < (SNTC_DBG(a, 128) ? 0 : 6); ++ct) {   // output channels 32 ct ... 32 ct + 31
        float* w2s = ring + (ct & 1) * 3072;
#pragma unroll
        for (int u = 0; u < 3; ++u) reinterpret_cast<f32x4*>(w2s)[te + 256 * u] = wreg[u];
        __syncthreads();                             // (the other buffer's readers are a tile behind this barrier)
        if (ct < 5) {
#pragma unroll
          for (int u = 0; u < 3; ++u) wreg[u] = w2src[(ct + 1) * 768 + te + 256 * u];
        }
        const int ch = 32 * ct + c4;
        f32x4 rv[4];
#pragma unroll
        for (int p = 0; p < 4; ++p) {
          rv[p] = f32x4{0.f, 0.f, 0.f, 0.f};
          if (a.epi != SNTC_EPI_STORE && mrow + 8 * p < a.M)
            rv[p] = *reinterpret_cast<const f32x4*>(a.res + (size_t)(mrow + 8 * p) * a.Cout2 + ch);
        }
        f32x16 acc2;
#pragma unroll
        for (int e = 0; e < 16; ++e) acc2[e] = 0.0f;
#pragma unroll
        for (int j = 0; j < 3; ++j)
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const f32x4 bq = *reinterpret_cast<const f32x4*>(w2s + ((4 * j + q) * 64 + lane) * 4);
#pragma unroll
            for (int e = 0; e < 4; ++e)
              acc2 = __builtin_amdgcn_mfma_f32_32x32x2f32(acc[0][j][4 * q + e], bq[e], acc2, 0, 0, 0);
          }
#pragma unroll
        for (int r = 0; r < 16; ++r) stage[((r & 3) + 8 * (r >> 2) + 4 * h) * 32 + l31] = acc2[r];
        f32x4 bv = {0.f, 0.f, 0.f, 0.f};
        if (a.bias2) bv = *reinterpret_cast<const f32x4*>(a.bias2 + ch);
#pragma unroll
        for (int p = 0; p < 4; ++p) {
          const int m = mrow + 8 * p;
          if (m >= a.M) continue;
          const size_t idx = (size_t)m * a.Cout2 + ch;         // forward convolution: the output pixel index is the row index
          f32x4 v = *reinterpret_cast<const f32x4*>(stage + (rsub + 8 * p) * 32 + c4) + bv;
          if (a.epi != SNTC_EPI_STORE) v = apply_epilogue(v, a.epi, rv[p], a.aux, idx);
          *reinterpret_cast<f32x4*>(a.y + idx) = v;
        }
      }
    } else if ((a.Cout & 3) == 0) {
      // Wide path (Cout % 4 == 0): each wave transposes its accumulators through a private LDS slice (the stage
      // ring is idle after the last barrier) so that every lane owns 4 consecutive channels of one pixel: bias /
      // residual / gate operands are read and the output is written with 16-B accesses.
      float* stage = ring + (DMA ? RING * SLOT - 4 * EPW : 0) + wave * EPW;
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j0 = 0; j0 < TN; j0 += 2) {
        const int ct = (TN - j0) >= 2 ? 2 : 1;          // tiles in this chunk
        const int wfl = ct * 32;                         // chunk width in floats
#pragma unroll
        for (int jj = 0; jj < 2; ++jj) {
          if (jj < ct) {
#pragma unroll
            for (int r = 0; r < 16; ++r)
              stage[((r & 3) + 8 * (r >> 2) + 4 * h) * wfl + jj * 32 + l31] = acc[i][j0 + jj][r];
          }
        }
        const int lanes_per_row = wfl >> 2;              // 16 or 8
        const int rows_per_pass = 64 / lanes_per_row;    // 4 or 8
        const int c4 = (lane % lanes_per_row) << 2;
        const int rsub = lane / lanes_per_row;
        const int col = n0d + (wn * TN + j0) * 32 + c4;
        const bool col_ok = col < Gd.Ncol;
        unsigned ce = 0;
        f32x4 bv = {0.f, 0.f, 0.f, 0.f};
        if (col_ok) {
          ce = Gd.cols[col];
          if (a.bias) bv = *reinterpret_cast<const f32x4*>(a.bias + (ce & 0xffff));
        }
        const int ch = ce & 0xffff;
        const int oyo = (int)((ce >> 24) & 0xff) - 128;
        const int oxo = (int)((ce >> 16) & 0xff) - 128;
        for (int rp = 0; rp < 32; rp += rows_per_pass) {
          const int rloc = rp + rsub;
          const int4 ri = rinfo[(wm * TM + i) * 32 + rloc];
          const int oy = ri.y * a.sO + oyo;
          const int ox = ri.z * a.sO + oxo;
          if (!col_ok || !ri.w || (unsigned)oy >= (unsigned)a.Ho || (unsigned)ox >= (unsigned)a.Wo) continue;
          const size_t idx = (((size_t)ri.x * a.Ho + oy) * a.Wo + ox) * a.Cout + ch;
          f32x4 v = *reinterpret_cast<const f32x4*>(stage + rloc * wfl + c4) + bv;
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] = apply_act(v[e], a.act);
          if (a.epi != SNTC_EPI_STORE)
            v = apply_epilogue(v, a.epi, SNTC_DBG(a, 32) ? v : *reinterpret_cast<const f32x4*>(a.res + idx), a.aux, idx);
          if (!SNTC_DBG(a, 16) || v[0] == 12345.678f) *reinterpret_cast<f32x4*>(a.y + idx) = v;
        }
      }
    } else {
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        const int col = n0d + (wn * TN + j) * 32 + l31;
        if (col >= Gd.Ncol) continue;
        const unsigned ce = Gd.cols[col];
        const int ch = ce & 0xffff;
        const int oyo = (int)((ce >> 24) & 0xff) - 128;
        const int oxo = (int)((ce >> 16) & 0xff) - 128;
        const float bv = a.bias ? a.bias[ch] : 0.0f;
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int row = (wm * TM + i) * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
          const int4 ri = rinfo[row];
          if (!ri.w) continue;
          const int oy = ri.y * a.sO + oyo;
          const int ox = ri.z * a.sO + oxo;
          if ((unsigned)oy >= (unsigned)a.Ho || (unsigned)ox >= (unsigned)a.Wo) continue;
          const size_t idx = (((size_t)ri.x * a.Ho + oy) * a.Wo + ox) * a.Cout + ch;
          a.y[idx] = apply_epilogue1(apply_act(acc[i][j][r] + bv, a.act), a.epi, a.res, a.aux, idx);
        }
      }
    }
    if (!more) break;
    __syncthreads();          // epilogue staging reads done before the next piece's stages land in the ring
    P = Q;
    rb = qb;
  }
}

// ---- the instantiations the library ships, one translation unit per mode (a new mode gets a file of its own: the fp32
// instances that carry the decode are then not even recompiled, and tools/kernel_resources.py pins their register allocation).
//   X(TM, TN, WM, WN): tile variants 1..7 (128 x 32 v), 8 (64 x 64), 9 (128 x 128), 10 (256 x 128)
#define SNTC_GG_SHAPES(X) X(1, 1, 4, 1) X(1, 2, 4, 1) X(1, 3, 4, 1) X(1, 4, 4, 1) X(1, 5, 4, 1) X(1, 6, 4, 1) X(1, 7, 4, 1) X(1, 1, 2, 2) X(2, 2, 2, 2) X(2, 4, 4, 1)
#define SNTC_GG_DMA_SHAPES(X) X(1, 1, 4, 1) X(1, 2, 4, 1) X(1, 3, 4, 1) X(1, 4, 4, 1) X(1, 5, 4, 1) X(1, 1, 2, 2) X(2, 2, 2, 2)
constexpr int kDeepRing = 8;   // ring slots of the deep direct-to-LDS instance (64 x 64)

}  // namespace sntc
