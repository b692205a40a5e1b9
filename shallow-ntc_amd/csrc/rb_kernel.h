// rb_kernel.h -- the whole-ResidualBlock kernel's tile walk, once: rb_body<C, A> is everything of the kernel that is not
// arithmetic (the persistent tile range, the LDS-DMA weight stream, the head's geometry on the halo patch and its epilogue into
// the patch ring, the frames of the 3x3 and of the transposed tail), templated on an arithmetic policy A that owns a unit's
// layout, the weight and pixel fragment registers and the MFMA sequence of every step with its schedule:
//   Fp32Arith (rb_fused.hip)       exact fp32, bit-identical to the three gather-GEMM launches;
//   Bf3Arith  (rb_fused_bf3.hip)   bf16 x 3 split precision.
// A policy is plain per-lane state with forced-inline members: nothing of it survives compilation but the registers it names.
// It keeps no copy of the body's lane ids (the body hands h to the members that need it): a copy moved the fp32 kernel's
// register allocation (profiles/rb_merge_resources.txt).  The __global__ kernels of the two files are the two instantiations.  A policy supplies
//   kUnitBytes                       bytes of a unit of the weight stream (a whole number of 1-KB LDS-DMA pieces)
//   kLaneHalf, kLoad2                head: byte offset of lane half h within a pixel's 64-B K stage, and of the lane's second load
//   chunk(sel, h)                    3x3: the 16-B chunk of a patch pixel's slab that fragment read `sel` of lane half h takes
//   init, prime                      fragment offsets; the first fragments of unit 0
//   head_begin, head_stage           one K stage of the head, from the fragment reads to the register rotation
//   conv_begin, conv_tap             one tap of the 3x3
//   tail_begin, tail_step            relu(acc + b1) as the tail's operand; one unit (half of K) of a 32-channel output tile
//   kSetupBeforeLastStep, kVm*       the end-of-tile hand-off, a measured schedule per policy (see the tail)
#pragma once
#include "rb_common.h"

namespace sntc {
namespace rb {

#ifdef SNTC_DIAG
// make DIAG=1: cycles per phase (s_memtime around head / 3x3 / tail, summed over the workgroup's tiles) overwrite the first
// floats of y at the end of the launch -- tools/rb_phases.py reads them; results are meaningless in such a build
#define RB_STAMP(v) const unsigned long long v = __builtin_amdgcn_s_memtime()
#else
#define RB_STAMP(v)
#endif

template <int V>
using IC = std::integral_constant<int, V>;

template <int C, class A>
__device__ __forceinline__ void rb_body(const RBArgs& a) {
  using K = RBCfg<C>;
  static_assert(A::C == C, "the policy's unit layout is that of this width");
  constexpr int CH = K::CH, NT = K::NT, SL = K::SL, PW = K::PW, PP = K::PP, PH = K::PH, NEW = K::TH * K::PW;
  constexpr int U0 = K::U0, U1 = K::U1, UT = K::UT, RING = K::RING, UNITB = A::kUnitBytes;
  static_assert(UNITB % 1024 == 0, "a unit is a whole number of 1-KB LDS-DMA pieces (64 lanes x 16 B)");
  typedef __attribute__((address_space(3))) void lds_void;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* patch = reinterpret_cast<float*>(smem);                    // [SL][PP][16] fp32, 16-B chunks XOR-swizzled by (pixel >> 2) & 3
  char* ring = smem + (size_t)K::PATCH * 4;                         // [RING] packed units as they are
  float* lbias = reinterpret_cast<float*>(ring + RING * UNITB);     // b0 | b1 | b2

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int l31 = lane & 31;
  const int h = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);

  // this workgroup's contiguous range of tiles; workgroups b, b + 8, ... (one XCD under round-robin placement) own one
  // contiguous eighth of the launch, so the halo rows neighbouring tiles share are L2 hits (speed only)
  const int G = gridDim.x, b = blockIdx.x;
  const int wl = (G & 7) == 0 ? (b & 7) * (G >> 3) + (b >> 3) : b;
  const int t_lo = (int)((long long)a.ntiles * wl / G);
  const int t_hi = (int)((long long)a.ntiles * (wl + 1) / G);
  if (t_lo >= t_hi) return;

  const __amdgpu_buffer_rsrc_t xs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.x), 0, (int)a.bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t ys = __builtin_amdgcn_make_buffer_rsrc(a.y, 0, (int)a.bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t ws =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.wpack), 0, UT * UNITB, 0x00020000);

  A ar;
  ar.init(ring, l31, h);

  // unit `unit` (of the stream, already wrapped) -> ring slot `slot`: a linear copy in 1-KB pieces (one wave instruction,
  // 16 B per lane), piece i by wave i % 8
  const unsigned dma_voff = (unsigned)lane * 16u;
  auto dma = [&](int unit, int slot) {
#pragma unroll
    for (int i = 0; i < UNITB / 1024; i += 8) {
      if (i + wave < UNITB / 1024) {
        char* dst = ring + slot * UNITB + (i + wave) * 1024;
        __builtin_amdgcn_raw_ptr_buffer_load_lds(ws, (lds_void*)dst, 16, (int)dma_voff, unit * UNITB + (i + wave) * 1024, 0, 0);
      }
    }
    __builtin_amdgcn_sched_barrier(0);
  };

  // the barrier of a step: everything this wave has in flight has landed (VM = accesses the wave may leave outstanding), then
  // the workgroup barrier publishes the unit the step's DMA brought (it is consumed two steps later, prefetched from one later)
  auto sync = [&](auto VM) {
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(decltype(VM)::value) : "memory");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
  };

  // ---- once per workgroup: biases into LDS, units 0 and 1 into the ring
  for (int i = tid; i < K::BIAS; i += 512) lbias[i] = a.bias[i];
  dma(0, 0);
  dma(1, 1);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();

  ar.prime();

  // Tiles are walked DOWN the image (column-major inside an image), and the patch is a ring of PH rows: image row r lives in
  // patch row (r + 1) % PH.  A tile right below the one this workgroup has just finished finds its two top halo rows in
  // place and computes only its 8 new rows (8 x 34 = 272 patch pixels instead of 340: 9 fragment tiles instead of 11) --
  // "incremental"; the first tile of a workgroup and the top tile of every column compute all ten -- "full".
  // Head work of this wave, in fragment tiles of 32 flat patch pixels f = 32 t + l31 -> (f / PW, f % PW) of the rows computed:
  //   full:        tile `wave` (all three channel tiles) and, waves 0 .. NPT - 9, tile `wave + 8` (all three)
  //   incremental: tile `wave` (all three) and, waves 0 .. NT - 1, channel tile `wave` of tile 8 (the 16 leftover pixels)
  const bool two = wave < K::NPT - 8;
  static_assert(K::NPT - 8 == NT, "the same waves take the second tile (full) and one channel tile of tile 8 (incremental)");
  int hf[3], hfy[3], hfx[3];                  // [0] tile wave, [1] tile wave + 8 (full), [2] tile 8 (incremental)
#pragma unroll
  for (int p = 0; p < 3; ++p) {
    hf[p] = 32 * (p == 0 ? wave : p == 1 ? wave + 8 : 8) + l31;
    hfy[p] = hf[p] / PW;
    hfx[p] = hf[p] - hfy[p] * PW;
  }
  unsigned hv[2];                              // [0] tile wave, [1] the second tile of this wave in the mode of the tile
  bool hvalid[2], hin[2];
  int hpp[2];                                  // patch pixel the lane's result goes to
  bool h_inc = false;
  f32x4 X[3][2][2];                            // [K stage % 3][patch tile][the lane's two loads]: the pixel fragments travel two stages ahead
  int n = 0, y0 = 0, x0 = 0;
  auto coords = [&](int tile, int* tn, int* ty0, int* tx0, bool* inc) {
    const int per = a.tiles_x * a.tiles_y;
    *tn = tile / per;
    const int r = tile - *tn * per;
    const int txi = r / a.tiles_y;
    const int tyi = r - txi * a.tiles_y;
    *ty0 = tyi * K::TH;
    *tx0 = txi * K::TW;
    *inc = tile > t_lo && tyi > 0;
  };
  // the head's pixel offsets of tile `tile` and its first two K stages on the way (issued a step before the tile begins)
  auto head_setup = [&](int tile) {
    int tn, ty0, tx0;
    coords(tile, &tn, &ty0, &tx0, &h_inc);
    const int r0 = h_inc ? 2 : 0;
    const int ybase = ty0 % PH + r0;             // patch row of the first row computed, before the wrap
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      const int q = p == 0 ? 0 : (h_inc ? 2 : 1);
      const int fy = hfy[q], fx = hfx[q];
      const int iy = ty0 - 1 + r0 + fy, ix = tx0 - 1 + fx;
      int pr = ybase + fy;
      pr = pr >= PH ? pr - PH : pr;
      pr = pr >= PH ? pr - PH : pr;
      hin[p] = hf[q] < (h_inc ? NEW : PP);
      hvalid[p] = hin[p] && (unsigned)iy < (unsigned)a.H && (unsigned)ix < (unsigned)a.W;
      hv[p] = hvalid[p] ? ((unsigned)((tn * a.H + iy) * a.W + ix) * (unsigned)(C * 4) + (unsigned)h * (unsigned)A::kLaneHalf) : kOOB;
      hpp[p] = pr * PW + fx;
    }
#pragma unroll
    for (int st = 0; st < 2; ++st) {
      X[st][0][0] = buf_load(xs, hv[0], st * 64);
      X[st][0][1] = buf_load(xs, hv[0], st * 64 + A::kLoad2);
      if (two) {
        X[st][1][0] = buf_load(xs, hv[1], st * 64);
        X[st][1][1] = buf_load(xs, hv[1], st * 64 + A::kLoad2);
      }
    }
  };
  head_setup(t_lo);

#ifdef SNTC_DIAG
  unsigned long long tph[4] = {0, 0, 0, 0};
#endif
  for (int tile = t_lo; tile < t_hi; ++tile) {
    bool inc_now;
    coords(tile, &n, &y0, &x0, &inc_now);
    RB_STAMP(ts0);

    // ================================================================================================
    // head: t1 = relu(W0 x + b0) on the halo patch, zero outside the image
    // ================================================================================================
    auto head = [&](auto NPXc, auto EXc) {
      constexpr int NPX = decltype(NPXc)::value;          // fragment tiles with all NT channel tiles
      constexpr bool EX = decltype(EXc)::value;           // + channel tile `wave` of one more fragment tile (its data in slot 1)
      constexpr int NLD = NPX + (EX ? 1 : 0);             // fragment tiles whose pixels this wave loads
      f32x16 acc[NT][NPX], accx;
#pragma unroll
      for (int e = 0; e < 16; ++e) accx[e] = 0.0f;
#pragma unroll
      for (int j = 0; j < NT; ++j)
#pragma unroll
        for (int p = 0; p < NPX; ++p)
#pragma unroll
          for (int e = 0; e < 16; ++e) acc[j][p][e] = 0.0f;
      ar.template head_begin<NLD>(X);
      static_for<0, U0>([&](auto J) {
        constexpr int j = decltype(J)::value;
        constexpr bool last = j == U0 - 1;
        // the pixel fragments of stage j + AHEAD are issued in step j (stages 0 and 1 came with head_setup): one step (1.5 us) is
        // not always enough for a first touch of x in HBM, two are; the two-tile variant (the first tile of a column, 1 in 32)
        // has no registers for a third buffer and stays one stage ahead
        constexpr int AHEAD = NPX == 2 ? 1 : 2;
        constexpr bool ld = j + AHEAD < U0 && j + AHEAD >= 2;
        dma(j + 2, (j + 2) % RING);
        if constexpr (ld) {
#pragma unroll
          for (int p = 0; p < NLD; ++p) {
            X[(j + AHEAD) % 3][p][0] = buf_load(xs, hv[p], (j + AHEAD) * 64);
            X[(j + AHEAD) % 3][p][1] = buf_load(xs, hv[p], (j + AHEAD) * 64 + A::kLoad2);
          }
        }
        ar.template head_stage<j, NPX, EX, ld>(acc, accx, X, wave);
        if constexpr (last) {
          // registers 4 q .. 4 q + 3 of tile jt = channels 32 jt + 8 q + 4 h + (0..3) of pixel l31: chunk 2 (q & 1) + h of slab 2 jt + (q >> 1)
          auto to_patch = [&](const f32x16& r, int jt, int p) {
            const int sw = (hpp[p] >> 2) & 3;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
              const f32x4 bv = *reinterpret_cast<const f32x4*>(lbias + 32 * jt + 8 * q + 4 * h);
              f32x4 v;
#pragma unroll
              for (int e = 0; e < 4; ++e) v[e] = hvalid[p] ? fmaxf(r[4 * q + e] + bv[e], 0.0f) : 0.0f;
              if (hin[p])
                *reinterpret_cast<f32x4*>(patch + (2 * jt + (q >> 1)) * (PP * 16) + hpp[p] * 16 + (((2 * (q & 1) + h) ^ sw) << 2)) = v;
            }
          };
#pragma unroll
          for (int p = 0; p < NPX; ++p)
#pragma unroll
            for (int jt = 0; jt < NT; ++jt) to_patch(acc[jt][p], jt, p);
          if constexpr (EX) to_patch(accx, wave, NPX);
        }
        if constexpr (ld && AHEAD == 2) sync(IC<2 * NLD>{});   // stage j + 2's fragments stay in flight across the barrier
        else sync(IC<0>{});
      });
    };
    using Yes = std::integral_constant<bool, true>;
    using No = std::integral_constant<bool, false>;
    if (!two) head(IC<1>{}, No{});
    else if (inc_now) head(IC<1>{}, Yes{});
    else head(IC<2>{}, No{});

    // ================================================================================================
    // 3x3: wave w = tile row w, lane = pixel, registers = the c/2 output channels
    // ================================================================================================
    RB_STAMP(ts1);
    f32x16 acc[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[j][e] = 0.0f;
    int bpp[3];                                // tap row dy of tile row `wave`: image row y0 - 1 + wave + dy, patch row (y0 + wave + dy) % PH
#pragma unroll
    for (int dy = 0; dy < 3; ++dy) bpp[dy] = ((y0 + wave + dy) % PH) * PW + l31;
    auto px_off = [&](int tap, int sel) {
      const int p = bpp[tap / 3] + (tap % 3);
      return p * 16 + (((A::chunk(sel, h) ^ ((p >> 2) & 3))) << 2);
    };
    ar.conv_begin(patch, px_off);
#pragma unroll 1
    for (int cc = 0; cc < SL; ++cc) {
      const float* pslab = patch + cc * (PP * 16);
      static_for<0, 9>([&](auto T) {
        constexpr int t = decltype(T)::value;
        dma(U0 + cc * 9 + t + 2, (t + 2) % RING);          // < UT: the last units belong to the tail
        ar.template conv_tap<t>(acc, patch, pslab, cc, px_off);
        sync(IC<0>{});
      });
    }

    // ================================================================================================
    // tail: y = x + W2 relu(acc + b1) + b2; the accumulators are the B operand
    // ================================================================================================
    RB_STAMP(ts2);
    ar.tail_begin(acc, lbias + CH, h);
    // output / residual addressing AFTER the quad transpose (rb_common.h): access j of an output tile is pixel 4 (l31 / 4) + j of
    // this wave's tile row, 16-B chunk 2 (l31 % 4) + h of its 32 channels
    const int oy = y0 + wave, ox4 = x0 + (l31 & ~3), li = l31 & 3;
    unsigned poff[4];
#pragma unroll
    for (int j = 0; j < 4; ++j)
      poff[j] = (oy < a.H && ox4 + j < a.W) ? ((unsigned)((n * a.H + oy) * a.W + ox4 + j) * (unsigned)(C * 4) + (unsigned)(2 * li + h) * 16u) : kOOB;
    static_for<0, C / 32>([&](auto OT) {
      constexpr int ot = decltype(OT)::value;
      f32x4 R[4];
      f32x16 acc2;
      static_for<0, 2>([&](auto HF) {
        constexpr int half = decltype(HF)::value;
        constexpr int u = U0 + U1 + 2 * ot + half;
        constexpr bool handoff = u == UT - 1;               // the tile's last step: the next tile's first K stages are issued here
        dma((u + 2) % UT, (u + 2) % RING);                  // wraps into the next tile's head (harmless after the last tile)
        if constexpr (half == 0) {
#pragma unroll
          for (int q = 0; q < 4; ++q) R[q] = buf_load(xs, poff[q], ot * 128);
#pragma unroll
          for (int e = 0; e < 16; ++e) acc2[e] = 0.0f;
        }
        if constexpr (handoff && A::kSetupBeforeLastStep) {
          if (tile + 1 < t_hi) head_setup(tile + 1);         // the next tile's first K stages travel under this step
          __builtin_amdgcn_sched_barrier(0);
        }
        ar.template tail_step<half, u>(acc, acc2);
        if constexpr (half == 1) {
          f32x4 T[4];
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const f32x4 bv = *reinterpret_cast<const f32x4*>(lbias + 2 * CH + 32 * ot + 8 * q + 4 * h);
            T[q] = f32x4{acc2[4 * q], acc2[4 * q + 1], acc2[4 * q + 2], acc2[4 * q + 3]} + bv;
          }
          quad_transpose(T, li);
#pragma unroll
          for (int j = 0; j < 4; ++j) buf_store(ys, T[j] + R[j], poff[j], ot * 128);
          if constexpr (handoff && !A::kSetupBeforeLastStep) {
            // the next tile's first two K stages are issued LAST, so that this step's wait can leave them (and the stores) in
            // flight: 4 stores + 4 loads per fragment tile
            __builtin_amdgcn_sched_barrier(0);
            if (tile + 1 < t_hi) {
              head_setup(tile + 1);
              if (two) sync(IC<A::kVmHandoffTwo>{});
              else sync(IC<A::kVmHandoffOne>{});
            } else {
              sync(IC<4>{});
            }
          } else {
            sync(IC<4>{});                                   // the four stores stay in flight
          }
        } else {
          sync(IC<A::kVmFirstHalf>{});
        }
      });
    });
#ifdef SNTC_DIAG
    RB_STAMP(ts3);
    tph[0] += ts1 - ts0; tph[1] += ts2 - ts1; tph[2] += ts3 - ts2; tph[3] += 1;
#endif
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#ifdef SNTC_DIAG
  __syncthreads();
  if (tid == 0)
    for (int k = 0; k < 4; ++k) a.y[blockIdx.x * 4 + k] = (float)tph[k];
#endif
}

}  // namespace rb
}  // namespace sntc
