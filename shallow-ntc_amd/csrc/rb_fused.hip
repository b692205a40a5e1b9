// rb_fused.hip -- the ELIC ResidualBlock (reference common/elic.py:41-68) as ONE launch on a 2-D pixel tile:
//
//     y = x + conv1x1_{c/2 -> c}( relu(conv3x3_{c/2 -> c/2}( relu(conv1x1_{c -> c/2}(x)) )) )
//
// A workgroup (512 threads = 8 waves, one per CU: the tile's patch fills the LDS) owns a tile of 8 rows x 32 pixels:
//   head   the 1x1 head on the (8+2) x (32+2) HALO patch, accumulated TRANSPOSED (weights = MFMA A operand, pixels = B
//          operand read straight from global memory, 16 B per lane): lane l then holds pixel l % 32 and four consecutive
//          channels per register quad -- one 16-B chunk of the patch's LDS image [16-channel slab][patch pixel][16], so
//          relu(acc + b0) goes to LDS with ds_write_b128 and out-of-image pixels become the 3x3's zero padding;
//   3x3    nine taps = nine SHIFTED fragment reads of that one patch (32 consecutive patch pixels per fragment: the
//          XOR swizzle stays conflict-free under any shift) -- no per-tap global gathers, no staging writes; wave w owns
//          tile row w and all c/2 output channels (lane = pixel, registers = channels);
//   tail   relu(acc + b1) is, as it stands in the registers, the B operand of the 1x1 tail (k = lane half, channel quads
//          in the fragment order of a 16-deep stage); the result leaves with bias, the skip (+ x) and 16-B stores.
// The three weight sets travel as ONE stream of 6-KB units (a unit = the LDS image of one 16-deep K stage of all c/2
// output rows) through a three-slot ring filled by LDS-DMA (buffer_load_dwordx4 ... lds, 1-KB pieces); the
// workgroup is persistent and the stream wraps from one tile's tail into the next tile's head.  Tiles are walked down the
// image and the patch is a ring of rows: a tile below the previous one re-uses its two top halo rows and computes 8 new ones.
//
// Every output element is the SAME k-ordered fp32 fma chain as in the three stand-alone gather-GEMM launches
// (gather_gemm.hip: stage = 16 channels, MFMA e of k-group g sums k in {8g+e, 8g+4+e}; 3x3: channel slab outermost,
// taps inside; products commute, zero padding contributes fma(0, w, acc)), so results are bit-identical to them.
//
// The tile walk itself is rb_body (rb_kernel.h), shared with the bf16 x 3 kernel of rb_fused_bf3.hip; this file holds the
// fp32 arithmetic policy, the fp32 pack kernel and the host code of both.
#include <algorithm>
#include <mutex>
#include "rb_kernel.h"

namespace sntc {
using namespace rb;

namespace {

#define RB_MFMA(a, b, c) __builtin_amdgcn_mfma_f32_32x32x2f32((a), (b), (c), 0, 0, 0)

// The exact fp32 arithmetic of rb_body (rb_kernel.h).  A unit is [CH rows][16 floats], its 16-B chunks XOR-swizzled by
// (row >> 2) & 3 (rb_pack_kernel below); a 32x32x2 operand is k = 8 g + 4 h + e in element e of k-group g.
struct Fp32Arith {
  using K = RBCfg<192>;
  static constexpr int C = 192, NT = K::NT, SL = K::SL, PP = K::PP, RING = K::RING, UNIT = K::UNIT;
  static constexpr int kUnitBytes = UNIT * 4;
  static constexpr int kLaneHalf = 16, kLoad2 = 32;       // a lane's two head loads: k-groups 0 and 1 of its half
  static __device__ __forceinline__ int chunk(int g, int h) { return 2 * g + h; }
  // end of tile: the next tile's head_setup goes BEFORE the last step's MFMAs, and every step's wait is the plain one
  static constexpr bool kSetupBeforeLastStep = true;
  static constexpr int kVmFirstHalf = 0, kVmHandoffTwo = 4, kVmHandoffOne = 4;   // the last two: not reached with the setup before the step

  const float* ring;
  int woff0, woff1;
  f32x4 Fw0[NT], Fw1[NT], FwN[NT];
  f32x4 Fp0, Fp1, FpN;

  // weight fragments: row = 32 j + l31 of the unit, 16-B chunk (2 g + h) ^ ((row >> 2) & 3): k = 8 g + 4 h + e in element e
  __device__ __forceinline__ void init(const char* ring_, int l31, int h) {
    ring = reinterpret_cast<const float*>(ring_);
    const int swz = (l31 >> 2) & 3;
    woff0 = l31 * 16 + (((0 + h) ^ swz) << 2);
    woff1 = l31 * 16 + (((2 + h) ^ swz) << 2);
  }
  __device__ __forceinline__ void read_w(f32x4 (&F)[NT], int slot, int g) {
    const float* base = ring + slot * UNIT + (g ? woff1 : woff0);
#pragma unroll
    for (int j = 0; j < NT; ++j) F[j] = *reinterpret_cast<const f32x4*>(base + j * 32 * 16);
  }
  __device__ __forceinline__ void prime() { read_w(Fw0, 0, 0); }

  template <int NLD>
  __device__ __forceinline__ void head_begin(const f32x4 (&)[3][2][2]) {}

  template <int j, int NPX, bool EX, bool ld>
  __device__ __forceinline__ void head_stage(f32x16 (&acc)[NT][NPX], f32x16& accx, const f32x4 (&X)[3][2][2], int wave) {
    constexpr int NLD = NPX + (EX ? 1 : 0);
    const int wxoff = wave * 32 * 16;                   // EX: the unit's row block of channel tile `wave`
    read_w(Fw1, j % RING, 1);
    f32x4 Fx0, Fx1;
    if constexpr (EX) {
      Fx0 = *reinterpret_cast<const f32x4*>(ring + (j % RING) * UNIT + wxoff + woff0);
      Fx1 = *reinterpret_cast<const f32x4*>(ring + (j % RING) * UNIT + wxoff + woff1);
    }
#pragma unroll
    for (int e = 0; e < 4; ++e)
#pragma unroll
      for (int jt = 0; jt < NT; ++jt)
#pragma unroll
        for (int p = 0; p < NPX; ++p) acc[jt][p] = RB_MFMA(Fw0[jt][e], X[j % 3][p][0][e], acc[jt][p]);
    if constexpr (EX) {
#pragma unroll
      for (int e = 0; e < 4; ++e) accx = RB_MFMA(Fx0[e], X[j % 3][NPX][0][e], accx);
    }
    // every memory instruction behind an MFMA that covers its issue slot (mask 0x8 MFMA, 0x20 VMEM read, 0x100 DS read)
    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
    if constexpr (ld) __builtin_amdgcn_sched_group_barrier(0x020, 2 * NLD, 0);
    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
    __builtin_amdgcn_sched_group_barrier(0x100, NT + (EX ? 2 : 0), 0);
    __builtin_amdgcn_sched_group_barrier(0x008, 4 * NT * NPX + (EX ? 4 : 0) - 2, 0);
    read_w(FwN, (j + 1) % RING, 0);
#pragma unroll
    for (int e = 0; e < 4; ++e)
#pragma unroll
      for (int jt = 0; jt < NT; ++jt)
#pragma unroll
        for (int p = 0; p < NPX; ++p) acc[jt][p] = RB_MFMA(Fw1[jt][e], X[j % 3][p][1][e], acc[jt][p]);
    if constexpr (EX) {
#pragma unroll
      for (int e = 0; e < 4; ++e) accx = RB_MFMA(Fx1[e], X[j % 3][NPX][1][e], accx);
    }
    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
    __builtin_amdgcn_sched_group_barrier(0x100, NT, 0);
    __builtin_amdgcn_sched_group_barrier(0x008, 4 * NT * NPX + (EX ? 4 : 0) - 1, 0);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int jt = 0; jt < NT; ++jt) Fw0[jt] = FwN[jt];
  }

  template <class PxOff>
  __device__ __forceinline__ void conv_begin(const float* patch, const PxOff& px_off) {
    Fp0 = *reinterpret_cast<const f32x4*>(patch + px_off(0, 0));
  }

  template <int t, class PxOff>
  __device__ __forceinline__ void conv_tap(f32x16 (&acc)[NT], const float* patch, const float* pslab, int cc, const PxOff& px_off) {
    read_w(Fw1, t % RING, 1);
    Fp1 = *reinterpret_cast<const f32x4*>(pslab + px_off(t, 1));
#pragma unroll
    for (int e = 0; e < 4; ++e)
#pragma unroll
      for (int jt = 0; jt < NT; ++jt) acc[jt] = RB_MFMA(Fw0[jt][e], Fp0[e], acc[jt]);
    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
    __builtin_amdgcn_sched_group_barrier(0x100, NT + 1, 0);
    __builtin_amdgcn_sched_group_barrier(0x008, 4 * NT - 1, 0);
    read_w(FwN, (t + 1) % RING, 0);
    if constexpr (t < 8) FpN = *reinterpret_cast<const f32x4*>(pslab + px_off(t + 1, 0));
    else FpN = *reinterpret_cast<const f32x4*>(patch + min(cc + 1, SL - 1) * (PP * 16) + px_off(0, 0));
#pragma unroll
    for (int e = 0; e < 4; ++e)
#pragma unroll
      for (int jt = 0; jt < NT; ++jt) acc[jt] = RB_MFMA(Fw1[jt][e], Fp1[e], acc[jt]);
    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
    __builtin_amdgcn_sched_group_barrier(0x100, NT + 1, 0);
    __builtin_amdgcn_sched_group_barrier(0x008, 4 * NT - 1, 0);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int jt = 0; jt < NT; ++jt) Fw0[jt] = FwN[jt];
    Fp0 = FpN;
  }

  // relu(acc + b1) is, as it stands in the registers, the tail's B operand
  __device__ __forceinline__ void tail_begin(f32x16 (&acc)[NT], const float* b1, int h) {
#pragma unroll
    for (int jt = 0; jt < NT; ++jt)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const f32x4 bv = *reinterpret_cast<const f32x4*>(b1 + 32 * jt + 8 * q + 4 * h);
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[jt][4 * q + e] = fmaxf(acc[jt][4 * q + e] + bv[e], 0.0f);
      }
  }

  template <int half, int u>
  __device__ __forceinline__ void tail_step(const f32x16 (&acc)[NT], f32x16& acc2) {
    read_w(Fw1, u % RING, 1);
    read_w(FwN, (u + 1) % RING, 0);
    // K = c/2 in stage order: stage st = NT * half + s of this unit, k-groups g = 0, 1, element e
    static_for<0, 2 * NT>([&](auto SG) {
      constexpr int sg = decltype(SG)::value, s = sg >> 1, g = sg & 1, st = NT * half + s;
#pragma unroll
      for (int e = 0; e < 4; ++e) acc2 = RB_MFMA((g ? Fw1 : Fw0)[s][e], acc[st >> 1][8 * (st & 1) + 4 * g + e], acc2);
      if constexpr (sg == 0) {
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x100, NT, 0);
        if constexpr (half == 0) __builtin_amdgcn_sched_group_barrier(0x020, 4, 0);
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x100, NT, 0);
        __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);
      }
    });
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int jt = 0; jt < NT; ++jt) Fw0[jt] = FwN[jt];
  }
};

template <int C>
__global__ void __launch_bounds__(512, 2) rb_kernel(const RBArgs a) {
  rb_body<C, Fp32Arith>(a);
}

// wpack[u][row][16] in the ring's LDS image order, from the Keras kernels: w0 [1,1,C,CH], w1 [3,3,CH,CH], w2 [1,1,CH,C]
template <int C>
__global__ void __launch_bounds__(256) rb_pack_kernel(const float* __restrict__ w0, const float* __restrict__ w1,
                                                       const float* __restrict__ w2, float* __restrict__ wpack) {
  using K = RBCfg<C>;
  constexpr int CH = K::CH, NT = K::NT;
  const int total = K::UT * K::UNIT;
  for (int idx = blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += gridDim.x * blockDim.x) {
    const int u = idx / K::UNIT;
    const int rem = idx - u * K::UNIT;
    const int row = rem >> 4, pos = rem & 15;
    const int chunk = (pos >> 2) ^ ((row >> 2) & 3);
    const int k16 = chunk * 4 + (pos & 3);
    float v;
    if (u < K::U0) {
      v = w0[(size_t)(16 * u + k16) * CH + row];
    } else if (u < K::U0 + K::U1) {
      const int s = u - K::U0, cc = s / 9, t = s - cc * 9;
      v = w1[((size_t)t * CH + 16 * cc + k16) * CH + row];
    } else {
      const int s = u - K::U0 - K::U1, ot = s >> 1, half = s & 1;
      const int st = NT * half + (row >> 5);
      v = w2[(size_t)(16 * st + k16) * C + 32 * ot + (row & 31)];
    }
    wpack[idx] = v;
  }
}

__global__ void rb_bias_kernel(const float* b0, const float* b1, const float* b2, float* out, int ch, int c) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < ch) out[i] = b0 ? b0[i] : 0.0f;
  else if (i < 2 * ch) out[i] = b1 ? b1[i - ch] : 0.0f;
  else if (i < 2 * ch + c) out[i] = b2 ? b2[i - 2 * ch] : 0.0f;
}

constexpr int kMaxDev = 16;
struct RBDevice {
  std::once_flag once;
  int rc = SNTC_OK;
  int num_cus = 0;
};
RBDevice g_rbdev[kMaxDev];

int rb_init(int* num_cus) {
  int dev = 0;
  SNTC_HIP(hipGetDevice(&dev));
  if (dev < 0 || dev >= kMaxDev) return fail(SNTC_ERR_UNSUPPORTED, "device index beyond the ResidualBlock tables");
  RBDevice& D = g_rbdev[dev];
  std::call_once(D.once, [&] {
    D.rc = [&]() -> int {
      hipDeviceProp_t prop;
      SNTC_HIP(hipGetDeviceProperties(&prop, dev));
      D.num_cus = prop.multiProcessorCount;
      SNTC_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&rb_kernel<192>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                   (int)RBCfg<192>::LDS));
      SNTC_HIP(hipFuncSetAttribute(rb3_kernel_ptr(), hipFuncAttributeMaxDynamicSharedMemorySize, (int)rb3_lds_bytes()));
      return SNTC_OK;
    }();
  });
  *num_cus = D.num_cus;
  return D.rc;
}

}  // namespace
}  // namespace sntc

struct sntc_resblock_plan {
  int c = 0;
  int precision = 0;          // 0: exact fp32 (rb_fused.hip); 1: bf16 x 3 split precision (rb_fused_bf3.hip)
  float* wpack = nullptr;
  void* wpack3 = nullptr;     // the pre-split weight stream (precision 1 only)
  float* bias = nullptr;
  int max_workgroups = 0;     // 0: one per CU
};

using namespace sntc;

static int rb_pack(sntc_resblock_plan* p, const float* w0, const float* b0, const float* w1, const float* b1, const float* w2,
                   const float* b2, hipStream_t s) {
  using K = RBCfg<192>;
  hipLaunchKernelGGL(rb_pack_kernel<192>, dim3((K::UT * K::UNIT + 255) / 256), dim3(256), 0, s, w0, w1, w2, p->wpack);
  hipLaunchKernelGGL(rb_bias_kernel, dim3((K::BIAS + 255) / 256), dim3(256), 0, s, b0, b1, b2, p->bias, K::CH, 192);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return hip_fail(e, "ResidualBlock weight packing");
  if (p->wpack3) return rb3_pack(w0, w1, w2, p->wpack3, s);
  return SNTC_OK;
}

extern "C" int sntc_resblock_supported(int c) { return c == 192 ? 1 : 0; }

static void rb_free(sntc_resblock_plan* p) {
  if (p->wpack) (void)hipFree(p->wpack);
  if (p->wpack3) (void)hipFree(p->wpack3);
  if (p->bias) (void)hipFree(p->bias);
  delete p;
}

extern "C" int sntc_resblock_plan_create(int c, const float* w0, const float* b0, const float* w1, const float* b1,
                                         const float* w2, const float* b2, int precision, void* stream, sntc_resblock_plan** plan) {
  if (!plan || !w0 || !w1 || !w2) return fail(SNTC_ERR_BAD_SHAPE, "sntc_resblock_plan_create: null argument");
  if (!sntc_resblock_supported(c)) return fail(SNTC_ERR_UNSUPPORTED, "sntc_resblock_plan_create: fused ResidualBlock exists for c = 192");
  if (precision != 0 && precision != 1) return fail(SNTC_ERR_UNSUPPORTED, "sntc_resblock_plan_create: precision 0 (fp32) or 1 (bf16 x 3)");
  int cus = 0;
  if (int rc = rb_init(&cus)) return rc;
  using K = RBCfg<192>;
  auto* p = new sntc_resblock_plan();
  p->c = c;
  p->precision = precision;
  if (hipMalloc(&p->wpack, sizeof(float) * K::UT * K::UNIT) != hipSuccess || hipMalloc(&p->bias, sizeof(float) * K::BIAS) != hipSuccess ||
      (precision == 1 && hipMalloc(&p->wpack3, rb3_pack_bytes()) != hipSuccess)) {
    rb_free(p);
    return fail(SNTC_ERR_HIP, "sntc_resblock_plan_create: out of device memory");
  }
  if (int rc = rb_pack(p, w0, b0, w1, b1, w2, b2, (hipStream_t)stream)) {
    rb_free(p);
    return rc;
  }
  *plan = p;
  return SNTC_OK;
}

extern "C" int sntc_resblock_plan_update(sntc_resblock_plan* p, const float* w0, const float* b0, const float* w1, const float* b1,
                                         const float* w2, const float* b2, void* stream) {
  if (!p || !w0 || !w1 || !w2) return fail(SNTC_ERR_BAD_SHAPE, "sntc_resblock_plan_update: null argument");
  return rb_pack(p, w0, b0, w1, b1, w2, b2, (hipStream_t)stream);
}

extern "C" void sntc_resblock_plan_destroy(sntc_resblock_plan* p) {
  if (p) rb_free(p);
}

extern "C" int sntc_resblock_plan_set_workgroups(sntc_resblock_plan* p, int max_workgroups) {
  if (!p || max_workgroups < 0) return fail(SNTC_ERR_BAD_SHAPE, "sntc_resblock_plan_set_workgroups: bad argument");
  p->max_workgroups = max_workgroups;
  return SNTC_OK;
}

extern "C" int64_t sntc_resblock_flops(const sntc_resblock_plan* p, int n, int h, int w) {
  if (!p || n < 0 || h < 0 || w < 0) return -1;
  const int64_t c = p->c, ch = p->c / 2;
  return 2 * (int64_t)n * h * w * (c * ch + 9 * ch * ch + ch * c);
}

extern "C" int sntc_resblock_forward(const sntc_resblock_plan* p, const float* x, int n, int h, int w, float* y, void* stream) {
  if (!p || !x || !y) return fail(SNTC_ERR_BAD_SHAPE, "sntc_resblock_forward: null argument");
  if (n < 0 || h < 0 || w < 0) return fail(SNTC_ERR_BAD_SHAPE, "sntc_resblock_forward: negative size");
  if (x == y) return fail(SNTC_ERR_BAD_SHAPE, "sntc_resblock_forward: y must not alias x (tiles read their neighbours' halo)");
  if (n == 0 || h == 0 || w == 0) return SNTC_OK;
  using K = RBCfg<192>;
  const int64_t bytes = (int64_t)n * h * w * p->c * 4;
  if (bytes >= (1LL << 31)) return fail(SNTC_ERR_BAD_SHAPE, "sntc_resblock_forward: tensor of 2 GiB or more; split the batch");
  int cus = 0;
  if (int rc = rb_init(&cus)) return rc;
  RBArgs a{};
  a.x = x; a.y = y; a.wpack = p->wpack; a.bias = p->bias;
  a.bytes = (unsigned)bytes;
  a.N = n; a.H = h; a.W = w;
  a.tiles_x = (w + K::TW - 1) / K::TW;
  a.tiles_y = (h + K::TH - 1) / K::TH;
  const int64_t nt = (int64_t)n * a.tiles_x * a.tiles_y;
  if (nt >= (1LL << 31)) return fail(SNTC_ERR_BAD_SHAPE, "sntc_resblock_forward: too many tiles");
  a.ntiles = (int)nt;
  int grid = std::min<int64_t>(nt, p->max_workgroups > 0 ? p->max_workgroups : cus);
  if (p->precision == 1) {
    a.wpack = reinterpret_cast<const float*>(p->wpack3);
    return rb3_launch(a, grid, (hipStream_t)stream);
  }
  hipLaunchKernelGGL(rb_kernel<192>, dim3(grid), dim3(512), K::LDS, (hipStream_t)stream, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return hip_fail(e, "ResidualBlock launch");
  return SNTC_OK;
}
