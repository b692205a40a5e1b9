// gather_gemm.hip -- host side of the gather GEMM: the split-K finish kernel, the table of compiled instances (defined in
// gg_inst_*.hip and bf3_gemm.hip), residency tables per device, the launch.
#include "gather_gemm_kernel.h"

namespace sntc {

// the instantiations live in their own translation units (gather_gemm_kernel.h, bottom); declared here so that the table
// below takes their addresses without instantiating them again
#define SNTC_GG_DECL_VEC(TM, TN, WM, WN) extern template __global__ void gg_kernel<TM, TN, WM, WN, true, false>(const GGArgs);
#define SNTC_GG_DECL_PRO(TM, TN, WM, WN)                                                   \
  extern template __global__ void gg_kernel<TM, TN, WM, WN, true, true>(const GGArgs);    \
  extern template __global__ void gg_kernel<TM, TN, WM, WN, false, true>(const GGArgs);
#define SNTC_GG_DECL_DMA(TM, TN, WM, WN) extern template __global__ void gg_kernel<TM, TN, WM, WN, true, false, false, true>(const GGArgs);
SNTC_GG_SHAPES(SNTC_GG_DECL_VEC)
SNTC_GG_SHAPES(SNTC_GG_DECL_PRO)
SNTC_GG_DMA_SHAPES(SNTC_GG_DECL_DMA)
extern template __global__ void gg_kernel<1, 1, 2, 2, true, false, false, true, kDeepRing>(const GGArgs);
extern template __global__ void gg_kernel<1, 3, 4, 1, true, false, false, false, 0, true>(const GGArgs);
extern template __global__ void gg_kernel<2, 2, 2, 2, true, false, false, false, 0, false, true>(const GGArgs);
extern template __global__ void gg_kernel<1, 2, 4, 1, true, false, true>(const GGArgs);
extern template __global__ void gg_kernel<1, 4, 4, 1, true, false, true>(const GGArgs);

// Split-K finish: y = epilogue(act(sum_{s = 0..S-1} slab[g][s][m][col] + bias)), splits added in index
// order (deterministic; the K ranges depend only on the layer and the image shape, never on the batch).
__global__ void __launch_bounds__(256) gg_reduce_kernel(const GGArgs a) {
  const GGGroup G = a.g[blockIdx.y];
  const size_t total = (size_t)a.M * G.Ncol;
  const int per = a.Qh * a.Qw;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int m = (int)(i / G.Ncol);
    const int col = (int)(i - (size_t)m * G.Ncol);
    float v = 0.0f;
    for (int sp = 0; sp < a.ksplit; ++sp) v += a.slab[G.slab_off + (size_t)sp * total + i];
    const unsigned ce = G.cols[col];
    const int ch = ce & 0xffff;
    const int n = m / per;
    const int rem = m - n * per;
    const int qy = rem / a.Qw + G.q0y, qx = rem - (rem / a.Qw) * a.Qw + G.q0x;
    const int oy = qy * a.sO + (int)((ce >> 24) & 0xff) - 128;
    const int ox = qx * a.sO + (int)((ce >> 16) & 0xff) - 128;
    if ((unsigned)oy >= (unsigned)a.Ho || (unsigned)ox >= (unsigned)a.Wo) continue;
    const size_t idx = (((size_t)n * a.Ho + oy) * a.Wo + ox) * a.Cout + ch;
    v = apply_act(v + (a.bias ? a.bias[ch] : 0.0f), a.act);
    a.y[idx] = apply_epilogue1(v, a.epi, a.res, a.aux, idx);
  }
}

int gg_reduce_launch(const GGArgs& args, hipStream_t stream) {
  size_t most = 0;
  for (int gi = 0; gi < args.ngroups; ++gi) most = std::max(most, (size_t)args.M * args.g[gi].Ncol);
  int blocks = (int)std::min<size_t>((most + 255) / 256, 2048);
  hipLaunchKernelGGL(gg_reduce_kernel, dim3(blocks, args.ngroups), dim3(256), 0, stream, args);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return hip_fail(e, "split-K reduce launch");
  return SNTC_OK;
}

// ---------------------------------------------------------------------------------------------
// the instance table
// ---------------------------------------------------------------------------------------------
// One row per compiled instance.  Tile (32 TM WM x 32 TN WN), threads (64 WM WN) and the stream-K hand-off slab (every thread's
// TM x TN accumulator tiles of 16 floats) follow from the template arguments; the dynamic LDS from the ring the instance stages
// through, plus the tile's row table.
static GGInstance row(int v, GGLoad load, GGStage stage, GGForm form, int TM, int TN, int WM, int WN, const void* fn) {
  GGInstance r{v, load, stage, form, 32 * TM * WM, 32 * TN * WN, 64 * WM * WN, 0, (size_t)TM * TN * 16 * 64 * WM * WN, fn};
  const size_t rinfo = 2 * r.bm * sizeof(int4);
  if (form == kFormPresplitHalo)         // the activation patch buffers + the weight ring (three bf16 planes: 96 B per row)
    r.lds = (size_t)2 * kBf3PatchRounds * 512 * 16 + (size_t)(v == 12 ? kBf3DeepRing : 3) * r.bn * 96 + rinfo;
  else if (form == kFormBf3 || form == kFormPresplit)    // three slots of (BM + BN) rows of 96 B
    r.lds = (size_t)3 * (r.bm + r.bn) * 96 + rinfo;
  else                                   // fp32: three, four (direct-to-LDS) or kDeepRing slots of (BM + BN) rows of 64 B
    r.lds = (size_t)(stage == kStageDeep ? kDeepRing : stage == kStageDma ? 4 : 3) * (r.bm + r.bn) * kStage * sizeof(float) + rinfo;
  return r;
}

#define GG(v, load, stage, form, TM, TN, WM, WN, ...) \
  row(v, load, stage, form, TM, TN, WM, WN, reinterpret_cast<const void*>(&gg_kernel<TM, TN, WM, WN, __VA_ARGS__>))
#define GG_LOADERS(v, TM, TN, WM, WN)                                        \
  GG(v, kLoadVec, kStageRing, kFormPlain, TM, TN, WM, WN, true, false),      \
  GG(v, kLoadVecPro, kStageRing, kFormPlain, TM, TN, WM, WN, true, true),    \
  GG(v, kLoadGather, kStageRing, kFormPlain, TM, TN, WM, WN, false, true)
#define GG_DMA(v, TM, TN, WM, WN) GG(v, kLoadVec, kStageDma, kFormPlain, TM, TN, WM, WN, true, false, false, true)
// bf3_kernel<WM = 4, WN = 2, TM = 2, TN, ...>: eight waves of 64 x 32 TN (bf3_gemm.hip)
#define BF3P(v, TN, form) row(v, kLoadVec, kStageDma, form, 2, TN, 4, 2, bf3p_kernel(v, form == kFormPresplitHalo))

static const GGInstance kInstances[] = {
    GG_LOADERS(1, 1, 1, 4, 1), GG_LOADERS(2, 1, 2, 4, 1), GG_LOADERS(3, 1, 3, 4, 1), GG_LOADERS(4, 1, 4, 4, 1), GG_LOADERS(5, 1, 5, 4, 1),
    GG_LOADERS(6, 1, 6, 4, 1), GG_LOADERS(7, 1, 7, 4, 1), GG_LOADERS(8, 1, 1, 2, 2), GG_LOADERS(9, 2, 2, 2, 2), GG_LOADERS(10, 2, 4, 4, 1),
    GG_DMA(1, 1, 1, 4, 1), GG_DMA(2, 1, 2, 4, 1), GG_DMA(3, 1, 3, 4, 1), GG_DMA(4, 1, 4, 4, 1), GG_DMA(5, 1, 5, 4, 1),
    GG_DMA(8, 1, 1, 2, 2), GG_DMA(9, 2, 2, 2, 2),
    // 8-slot ring (six stages in flight per workgroup) for launches of about one workgroup per CU or fewer, where nothing else
    // hides the memory latency: the 64 x 64 tile, which is what such launches are cut into
    GG(8, kLoadVec, kStageDeep, kFormPlain, 1, 1, 2, 2, true, false, false, true, kDeepRing),
    // the ResidualBlock tail fused behind the 128 x 96 tile (3x3, N = 96 -> 1x1, 96 -> 192)
    GG(3, kLoadVec, kStageRing, kFormFuse2, 1, 3, 4, 1, true, false, false, false, 0, true),
    // the column-tile-outermost twin of the 128 x 128 stream-K instance (GGArgs::order == 0; single-group plans)
    GG(9, kLoadVec, kStageRing, kFormColm, 2, 2, 2, 2, true, false, false, false, 0, false, true),
    GG(2, kLoadVec, kStageRing, kFormBf3, 1, 2, 4, 1, true, false, true),
    GG(4, kLoadVec, kStageRing, kFormBf3, 1, 4, 4, 1, true, false, true),
    BF3P(11, 4, kFormPresplit), BF3P(11, 4, kFormPresplitHalo), BF3P(12, 2, kFormPresplit), BF3P(12, 2, kFormPresplitHalo),
    BF3P(13, 3, kFormPresplit), BF3P(13, 3, kFormPresplitHalo),
};
#undef GG
#undef GG_LOADERS
#undef GG_DMA
#undef BF3P
constexpr int kNumInstances = sizeof(kInstances) / sizeof(kInstances[0]);

const GGInstance* gg_find(int variant, GGLoad load, GGStage stage, GGForm form) {
  for (const GGInstance& r : kInstances)
    if (r.variant == variant && r.load == load && r.stage == stage && r.form == form) return &r;
  return nullptr;
}

static bool presplit(const GGInstance& r) { return r.form == kFormPresplit || r.form == kFormPresplitHalo; }

// Residency tables, one per device, filled once per process (std::call_once): every thread and every plan sees the same
// schedule whatever thread created the plan, and switching devices costs a table lookup.
constexpr int kMaxDevices = 16;
struct DeviceTables {
  std::once_flag once;
  int rc = SNTC_OK;
  int num_cus = 0;
  int resident[kNumInstances] = {};            // workgroups per device, by row of kInstances
  int* status = nullptr;                       // sticky status word (device memory)
};
static DeviceTables g_dev[kMaxDevices];

static int fill_tables(DeviceTables& T, int dev) {
  hipDeviceProp_t prop;
  SNTC_HIP(hipGetDeviceProperties(&prop, dev));
  T.num_cus = prop.multiProcessorCount;
  for (int i = 0; i < kNumInstances; ++i) {
    const GGInstance& r = kInstances[i];
    SNTC_HIP(hipFuncSetAttribute(r.fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)r.lds));
    if (presplit(r)) {                         // one 512-thread workgroup per CU, by construction
      T.resident[i] = T.num_cus;
      continue;
    }
    int per_cu = 0;
    SNTC_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, r.fn, r.threads, r.lds));
    // the API can answer one workgroup per CU high near an SGPR allocation edge (MI355X_MICROARCH.md, Residency):
    // stream-K needs every worker resident, so stay at or below 8 and keep the LDS bound exact
    per_cu = std::max(1, std::min({per_cu, 8, (int)(163840 / r.lds)}));
    T.resident[i] = per_cu * T.num_cus;
  }
  SNTC_HIP(hipMalloc(&T.status, 2 * sizeof(int)));      // [0] the sticky word, [1] where sntc_conv_status's exchange returns it
  SNTC_HIP(hipMemset(T.status, 0, 2 * sizeof(int)));
  return SNTC_OK;
}

static DeviceTables* current_tables() {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kMaxDevices) return nullptr;
  DeviceTables& T = g_dev[dev];
  std::call_once(T.once, [&] { T.rc = fill_tables(T, dev); });
  return T.rc == SNTC_OK ? &T : nullptr;
}

int gg_init() {
  int dev = 0;
  SNTC_HIP(hipGetDevice(&dev));
  if (dev < 0 || dev >= kMaxDevices) return fail(SNTC_ERR_UNSUPPORTED, "device index beyond the residency tables");
  DeviceTables& T = g_dev[dev];
  std::call_once(T.once, [&] { T.rc = fill_tables(T, dev); });
  return T.rc;
}

int gg_resident(const GGInstance& inst) {
  const DeviceTables* T = current_tables();
  return T ? T->resident[&inst - kInstances] : 0;
}

int gg_num_cus() {
  const DeviceTables* T = current_tables();
  return T ? T->num_cus : 0;
}

int* gg_status_word() {
  const DeviceTables* T = current_tables();
  return T ? T->status : nullptr;
}

// The launch of one resolved instance: the mode fields of GGArgs are the instance's (the pre-split kernels take GGArgs::order
// from the caller: there it is the plan's A/B switch of the unit order, not an instance).
int gg_launch(const GGInstance& inst, const GGArgs& args, int nblocks, hipStream_t stream) {
  GGArgs a = args;
  a.dma = inst.stage;
  a.bf3 = inst.form == kFormBf3 || presplit(inst) ? 1 : 0;
  a.halo = inst.form == kFormPresplitHalo ? 1 : 0;
  if (!presplit(inst)) a.order = inst.form == kFormColm ? 0 : 1;
#ifdef SNTC_DIAG
  if (const char* e = getenv("SNTC_GG_DBG")) a.dbg = atoi(e);   // diagnostic builds only (make DIAG=1): results are WRONG with it
#endif
  void* params[] = {&a};
  hipError_t e = hipLaunchKernel(inst.fn, dim3(nblocks), dim3(inst.threads), params, inst.lds, stream);
  if (e != hipSuccess) return hip_fail(e, "gather-GEMM launch");
  return SNTC_OK;
}

}  // namespace sntc
