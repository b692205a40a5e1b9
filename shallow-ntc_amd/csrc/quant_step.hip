// quant_step.hip -- the latents of the mean-scale hyperprior quantised with a step off the scale ladder (DESIGN.md 4.7,
// "variable rate").  The 64 coding tables sit on sigma_i = 0.11 r^i, r = exp(kScaleFactor): a symbol round((y - mu) / r^k) of an
// element whose table would be i is distributed as table i - k describes, so the tables, the coder and the decoder serve every
// step k of the ladder unchanged.  Three rules, one device function each, shared by every kernel here (the symbol rule in its two
// halves, step_diff and step_round: the ladder kernel subtracts once per element and rounds once per candidate with the same code):
//   symbol    s = (int)rintf((y - mu) * inv_step)            float32 subtract, then float32 multiply
//   table id  t = clamp(t0 - k, 0, 63)                       t0 = sntc_scale_table_ids; off the ladder's ends the end table stays
//   value     y_hat = fmaf(step, (float)s, mu)
// The rules live in step_rules.h: SGA at a step (sga.hip) samples and dequantises with the same functions, and quant_step_map.hip
// applies all three with an index per latent position.
// At k = 0 (step = inv_step = 1.0f) they are the symbols of sntc_entropy_scale_normal, the ids of sntc_scale_table_ids and the
// values of sntc_dequant_mean, bit for bit.
//
// step_ladder_cost_kernel is rans_cost_kernel (rans_cost.hip) with the symbols formed on the fly for up to kLadderMax steps at
// once: y, mu and the base ids are read ONCE (10 bytes per element), every candidate's symbol is priced from the tables in LDS,
// and the sums stay integers from the lane to the atomic -- the result does not depend on the launch geometry.  Per element that
// is 2 K LDS reads (descriptor, price) against 10 bytes from memory: the launch is not HBM-bound (measured 0.76 TB/s at K = 16 on
// 8.8 M elements, 2.7 look-ups per clock and CU); by bank arithmetic neither LDS nor VALU issue is saturated, it is the dependent
// chain id -> descriptor -> symbol -> price across both pipes; no counter run has split the two.
#include <algorithm>
#include "rans_common.h"
#include "step_rules.h"

namespace sntc {

constexpr int kLadderMax = 16;                              // candidate steps of one ladder launch (their sums live in registers)
constexpr int kLadderThreads = 1024;
constexpr int kLadderGrid = 512;                            // workgroups of a launch, about
constexpr int kLadderLdsLimit = kRansLdsTotal;              // descriptors + cost_q staged in LDS up to here

__device__ __forceinline__ int step_symbol(float y, float mu, float inv_step) { return step_round(step_diff(y, mu), inv_step); }

typedef int qs_i32x4 __attribute__((ext_vector_type(4)));
typedef float qs_f32x4 __attribute__((ext_vector_type(4)));

// grid (blocks per image, n); one thread = 4 consecutive channels of a pixel per pass (c % 4 == 0)
__global__ void __launch_bounds__(256) step_symbols_kernel(const float* __restrict__ y, const float* __restrict__ mu,
                                                           const unsigned short* __restrict__ tid0, long long hw, int c, int mu_stride,
                                                           const float* __restrict__ inv_step, const int* __restrict__ shift,
                                                           int* __restrict__ symbols, unsigned short* __restrict__ tid) {
  const int img = blockIdx.y, c4 = c >> 2;
  const float inv = inv_step[img];
  const int k = shift[img];
  const long long nvec = hw * c4, base = (long long)img * hw * c;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < nvec; i += (long long)gridDim.x * blockDim.x) {
    const long long p = i / c4;
    const int ch = (int)(i - p * c4) << 2;
    const qs_f32x4 yv = *reinterpret_cast<const qs_f32x4*>(y + base + i * 4);
    const qs_f32x4 m = *reinterpret_cast<const qs_f32x4*>(mu + ((long long)img * hw + p) * mu_stride + ch);
    const ushort4 t = *reinterpret_cast<const ushort4*>(tid0 + base + i * 4);
    qs_i32x4 s;
#pragma unroll
    for (int e = 0; e < 4; ++e) s[e] = step_symbol(yv[e], m[e], inv);
    ushort4 o;
    o.x = (unsigned short)step_table_id(t.x, k);
    o.y = (unsigned short)step_table_id(t.y, k);
    o.z = (unsigned short)step_table_id(t.z, k);
    o.w = (unsigned short)step_table_id(t.w, k);
    *reinterpret_cast<qs_i32x4*>(symbols + base + i * 4) = s;
    *reinterpret_cast<ushort4*>(tid + base + i * 4) = o;
  }
}

// the decoder's half of step_symbols_kernel: it has the ids of the hyper-synthesis and no y
__global__ void __launch_bounds__(256) step_table_ids_kernel(const unsigned short* __restrict__ tid0, long long elems,
                                                             const int* __restrict__ shift, unsigned short* __restrict__ tid) {
  const int k = shift[blockIdx.y];
  const long long base = (long long)blockIdx.y * elems;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < elems; i += (long long)gridDim.x * blockDim.x)
    tid[base + i] = (unsigned short)step_table_id(tid0[base + i], k);
}

__global__ void __launch_bounds__(256) dequant_step_kernel(const int* __restrict__ symbols, const float* __restrict__ mu, long long hw,
                                                           int c, int mu_stride, const float* __restrict__ step,
                                                           float* __restrict__ y_hat) {
  const int img = blockIdx.y, c4 = c >> 2;
  const float st = step[img];
  const long long nvec = hw * c4, base = (long long)img * hw * c;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < nvec; i += (long long)gridDim.x * blockDim.x) {
    const long long p = i / c4;
    const int ch = (int)(i - p * c4) << 2;
    const qs_i32x4 s = *reinterpret_cast<const qs_i32x4*>(symbols + base + i * 4);
    const qs_f32x4 m = *reinterpret_cast<const qs_f32x4*>(mu + ((long long)img * hw + p) * mu_stride + ch);
    qs_f32x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = step_value(s[e], m[e], st);
    *reinterpret_cast<qs_f32x4*>(y_hat + base + i * 4) = o;
  }
}

// grid (workgroups per image, n): no workgroup straddles an image.  A thread's unit is V elements of one pixel (V = 4: one
// 16-byte load of y and of mu, 8 bytes of ids; V = 1 where a pointer is not aligned for that); (pixel, unit in the pixel)
// advance by the launch's stride as (dq, dr): no division in the loop.  nsteps <= kLadderMax candidates: inv_step / shift are
// uniform, their sums 64-bit per lane.
template <bool LDS, int V>
__global__ void __launch_bounds__(kLadderThreads) step_ladder_cost_kernel(const float* __restrict__ y, const float* __restrict__ mu,
                                                                          const unsigned short* __restrict__ tid0, long long hw, int c,
                                                                          int mu_stride, const float* __restrict__ inv_step,
                                                                          const int* __restrict__ shift, int nsteps, RansTables T,
                                                                          const unsigned* __restrict__ cost_q, int dq, int dr,
                                                                          unsigned long long* __restrict__ cost) {
  extern __shared__ unsigned char smem[];
  __shared__ unsigned long long partial[kLadderThreads / 64][kLadderMax];
  const uint2* meta = T.meta;
  const unsigned* cq = cost_q;
  if (LDS) {
    uint2* m = reinterpret_cast<uint2*>(smem);
    unsigned* q = reinterpret_cast<unsigned*>(smem + (size_t)T.ntables * sizeof(uint2));
    for (int i = threadIdx.x; i < T.ntables; i += kLadderThreads) m[i] = T.meta[i];
    for (int i = threadIdx.x; i < T.total; i += kLadderThreads) q[i] = cost_q[i];
    __syncthreads();
    meta = m;
    cq = q;
  }
  float inv[kLadderMax];
  int sh[kLadderMax];
  unsigned long long sum[kLadderMax];
#pragma unroll
  for (int k = 0; k < kLadderMax; ++k) {
    inv[k] = k < nsteps ? inv_step[k] : 0.0f;
    sh[k] = k < nsteps ? shift[k] : 0;
    sum[k] = 0ull;
  }
  const int img = blockIdx.y, cu = c / V;                    // units per pixel
  const long long nunit = hw * cu, base = (long long)img * hw * c;
  const long long stride = (long long)gridDim.x * kLadderThreads;
  const long long i0 = (long long)blockIdx.x * kLadderThreads + threadIdx.x;
  long long p = i0 / cu;
  int r = (int)(i0 - p * cu);
  for (long long i = i0; i < nunit; i += stride) {
    float d[V];
    unsigned t0[V];
    const float* yp = y + base + i * V;
    const float* mp = mu + ((long long)img * hw + p) * mu_stride + r * V;
    const unsigned short* tp = tid0 + base + i * V;
    if (V == 4) {
      const qs_f32x4 yv = *reinterpret_cast<const qs_f32x4*>(yp);
      const qs_f32x4 mv = *reinterpret_cast<const qs_f32x4*>(mp);
      const ushort4 tv = *reinterpret_cast<const ushort4*>(tp);
      const unsigned short ts[4] = {tv.x, tv.y, tv.z, tv.w};
#pragma unroll
      for (int e = 0; e < V; ++e) {
        d[e] = step_diff(yv[e], mv[e]);
        t0[e] = ts[e];
      }
    } else {
      d[0] = step_diff(yp[0], mp[0]);
      t0[0] = tp[0];
    }
#pragma unroll
    for (int k = 0; k < kLadderMax; ++k) {
      if (k < nsteps) {
        unsigned part = 0u;                                  // <= 4 x 2^22: an entry of cost_q is below (16 + 16) x 65536
#pragma unroll
        for (int e = 0; e < V; ++e) {
          const uint2 m = meta[step_table_id(t0[e], sh[k])];
          bool esc;
          const int sym = rans_symbol(step_round(d[e], inv[k]), m, esc);
          part += cq[m.x + sym];
        }
        sum[k] += part;
      }
    }
    p += dq;
    r += dr;
    if (r >= cu) {
      r -= cu;
      ++p;
    }
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < kLadderMax; ++k) {
    if (k < nsteps) {
      unsigned long long s = sum[k];
      for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off);
      if (lane == 0) partial[wave][k] = s;
    }
  }
  __syncthreads();
  if (threadIdx.x < nsteps) {
    unsigned long long s = 0ull;
    for (int w = 0; w < kLadderThreads / 64; ++w) s += partial[w][threadIdx.x];
    atomicAdd(&cost[(long long)img * nsteps + threadIdx.x], s);
  }
}

template <bool LDS, int V>
static int launch_ladder(dim3 grid, int lds, hipStream_t s, const float* y, const float* mu, const unsigned short* tid0, long long hw,
                         int c, int mu_stride, const float* inv_step, const int* shift, int nsteps, const RansTables& T,
                         const unsigned* cost_q, unsigned long long* cost) {
  if (LDS) SNTC_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(step_ladder_cost_kernel<LDS, V>), hipFuncAttributeMaxDynamicSharedMemorySize, lds));
  const long long stride = (long long)grid.x * kLadderThreads;
  const int cu = c / V;
  hipLaunchKernelGGL((step_ladder_cost_kernel<LDS, V>), grid, dim3(kLadderThreads), LDS ? lds : 0, s, y, mu, tid0, hw, c, mu_stride,
                     inv_step, shift, nsteps, T, cost_q, (int)(stride / cu), (int)(stride % cu), cost);
  SNTC_HIP(hipGetLastError());
  return SNTC_OK;
}

static bool step_sizes_ok(int n, int64_t hw, int c, int mu_stride) {
  return n >= 1 && n <= 65535 && hw >= 1 && c >= 1 && c % 4 == 0 && mu_stride >= c && mu_stride % 4 == 0;
}

static bool aligned(const void* p, uintptr_t a) { return reinterpret_cast<uintptr_t>(p) % a == 0; }

static unsigned step_blocks(int64_t nvec) { return (unsigned)std::min<int64_t>(std::max<int64_t>((nvec + 1023) / 1024, 1), 1024); }

}  // namespace sntc

using namespace sntc;

extern "C" int sntc_step_symbols(const float* y, const float* mu, int n, int64_t hw, int c, int mu_stride, const uint16_t* base_ids,
                                 const float* inv_step, const int32_t* shift, int32_t* symbols, uint16_t* table_ids, void* stream) {
  if (!y || !mu || !base_ids || !inv_step || !shift || !symbols || !table_ids)
    return fail(SNTC_ERR_BAD_SHAPE, "sntc_step_symbols: null argument");
  if (!step_sizes_ok(n, hw, c, mu_stride))
    return fail(SNTC_ERR_BAD_SHAPE, "sntc_step_symbols: bad sizes (1 <= n <= 65535, c % 4 == 0, mu_stride >= c, mu_stride % 4 == 0)");
  if (!aligned(y, 16) || !aligned(mu, 16) || !aligned(symbols, 16) || !aligned(base_ids, 8) || !aligned(table_ids, 8))
    return fail(SNTC_ERR_BAD_SHAPE, "sntc_step_symbols: y / mu / symbols must be 16-byte aligned, the id arrays 8-byte aligned");
  hipLaunchKernelGGL(step_symbols_kernel, dim3(step_blocks(hw * (c / 4)), n), dim3(256), 0, (hipStream_t)stream, y, mu, base_ids,
                     (long long)hw, c, mu_stride, inv_step, shift, symbols, table_ids);
  SNTC_HIP(hipGetLastError());
  return SNTC_OK;
}

extern "C" int sntc_step_table_ids(const uint16_t* base_ids, int n, int64_t elems_per_image, const int32_t* shift, uint16_t* table_ids,
                                   void* stream) {
  if (!base_ids || !shift || !table_ids) return fail(SNTC_ERR_BAD_SHAPE, "sntc_step_table_ids: null argument");
  if (n < 1 || n > 65535 || elems_per_image < 1) return fail(SNTC_ERR_BAD_SHAPE, "sntc_step_table_ids: bad sizes (1 <= n <= 65535)");
  hipLaunchKernelGGL(step_table_ids_kernel, dim3(step_blocks(elems_per_image / 4 + 1), n), dim3(256), 0, (hipStream_t)stream, base_ids,
                     (long long)elems_per_image, shift, table_ids);
  SNTC_HIP(hipGetLastError());
  return SNTC_OK;
}

extern "C" int sntc_dequant_step(const int32_t* symbols, const float* mu, int n, int64_t hw, int c, int mu_stride, const float* step,
                                 float* y_hat, void* stream) {
  if (!symbols || !mu || !step || !y_hat) return fail(SNTC_ERR_BAD_SHAPE, "sntc_dequant_step: null argument");
  if (!step_sizes_ok(n, hw, c, mu_stride))
    return fail(SNTC_ERR_BAD_SHAPE, "sntc_dequant_step: bad sizes (1 <= n <= 65535, c % 4 == 0, mu_stride >= c, mu_stride % 4 == 0)");
  if (!aligned(symbols, 16) || !aligned(mu, 16) || !aligned(y_hat, 16))
    return fail(SNTC_ERR_BAD_SHAPE, "sntc_dequant_step: symbols / mu / y_hat must be 16-byte aligned");
  hipLaunchKernelGGL(dequant_step_kernel, dim3(step_blocks(hw * (c / 4)), n), dim3(256), 0, (hipStream_t)stream, symbols, mu,
                     (long long)hw, c, mu_stride, step, y_hat);
  SNTC_HIP(hipGetLastError());
  return SNTC_OK;
}

extern "C" int sntc_step_ladder_cost(const float* y, const float* mu, int n, int64_t hw, int c, int mu_stride, const uint16_t* base_ids,
                                     const float* inv_step, const int32_t* shift, int nsteps, const uint32_t* meta, int ntables,
                                     int total_entries, const uint32_t* cost_q, uint64_t* cost, void* stream) {
  if (!y || !mu || !base_ids || !inv_step || !shift || !meta || !cost_q || !cost)
    return fail(SNTC_ERR_BAD_SHAPE, "sntc_step_ladder_cost: null argument");
  if (!step_sizes_ok(n, hw, c, mu_stride))
    return fail(SNTC_ERR_BAD_SHAPE, "sntc_step_ladder_cost: bad sizes (1 <= n <= 65535, c % 4 == 0, mu_stride >= c, mu_stride % 4 == 0)");
  if (nsteps < 1 || nsteps > kLadderMax) return fail(SNTC_ERR_BAD_SHAPE, "sntc_step_ladder_cost: 1 <= nsteps <= 16");
  if (ntables <= kLadderTop || total_entries < 1)
    return fail(SNTC_ERR_BAD_SHAPE, "sntc_step_ladder_cost: the table set must hold the 64 tables of the scale ladder");
  if (!aligned(y, 4) || !aligned(mu, 4) || !aligned(base_ids, 2) || !aligned(cost, 8))
    return fail(SNTC_ERR_BAD_SHAPE, "sntc_step_ladder_cost: misaligned argument");
  hipStream_t s = (hipStream_t)stream;
  if (int zrc = zero_async(cost, (size_t)n * nsteps * sizeof(uint64_t), s)) return zrc;
  const RansTables T{nullptr, reinterpret_cast<const uint2*>(meta), ntables, total_entries};   // the price replaces the cdf: never read
  const bool vec = aligned(y, 16) && aligned(mu, 16) && aligned(base_ids, 8);
  const long long nunit = (long long)hw * (c / (vec ? 4 : 1));
  const long long want = (nunit + kLadderThreads - 1) / kLadderThreads, most = std::max<long long>(1, kLadderGrid / n);
  const dim3 grid((unsigned)std::min(want, most), (unsigned)n);
  const long long tb = (long long)ntables * (long long)sizeof(uint2) + 4LL * total_entries;
  const bool lds = tb <= kLadderLdsLimit;
  unsigned long long* out = reinterpret_cast<unsigned long long*>(cost);
  const int* sh = reinterpret_cast<const int*>(shift);
  if (lds && vec) return launch_ladder<true, 4>(grid, (int)tb, s, y, mu, base_ids, hw, c, mu_stride, inv_step, sh, nsteps, T, cost_q, out);
  if (lds) return launch_ladder<true, 1>(grid, (int)tb, s, y, mu, base_ids, hw, c, mu_stride, inv_step, sh, nsteps, T, cost_q, out);
  if (vec) return launch_ladder<false, 4>(grid, 0, s, y, mu, base_ids, hw, c, mu_stride, inv_step, sh, nsteps, T, cost_q, out);
  return launch_ladder<false, 1>(grid, 0, s, y, mu, base_ids, hw, c, mu_stride, inv_step, sh, nsteps, T, cost_q, out);
}
