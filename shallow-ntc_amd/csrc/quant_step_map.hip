// quant_step_map.hip -- quant_step.hip with the ladder index of the step varying per latent POSITION ("variable
// rate": region-of-interest coding, wire format 7).  All c channels of a position share one index k in [-32, 32]; at that index
// the three rules of step_rules.h hold unchanged:
//   symbol    s = step_round(step_diff(y, mu), inv_step(k))
//   table id  t = step_table_id(t0, k) = clamp(t0 - k, 0, 63)
//   value     y_hat = step_value(s, mu, step(k))
// step(k) / inv_step(k) are never computed here: the host uploads ONE table `lut`, float32 [2][65], row 0 = step, row 1 =
// inv_step, indexed by k + 32 (entropy_coding.step_size: float64, rounded once).  Every kernel clamps the index it reads into
// [-32, 32] first (map_index), so a stray byte in a map can never read outside the table; the host validates the maps anyway.
// With a constant map these are the symbols, ids, values and costs of quant_step.hip's per-image kernels at that index, bit
// for bit.
//
// step_map_ladder_cost_kernel is step_ladder_cost_kernel with candidate j's index at position p = clamp(base[j] + offsets[p]):
// a thread's unit is V channels of ONE position, so it reads one offset per unit and, per candidate, one inverse step from the
// 65 floats staged in LDS; y, mu and the ids are still read once per launch and the sums are integers from the lane to the
// atomic.
#include <algorithm>
#include "rans_common.h"
#include "step_rules.h"

namespace sntc {

// kMapMin / kMapMax / kMapLut and map_index: step_rules.h (the SGA map kernels of sga.hip read the same table)
constexpr int kMapLadderMax = 16;                           // candidate bases of one ladder launch (their sums live in registers)
constexpr int kMapLadderThreads = 1024;
constexpr int kMapLadderGrid = 512;                         // workgroups of a launch, about
constexpr int kMapLadderLdsLimit = kRansLdsTotal;           // descriptors + cost_q staged in LDS up to here

typedef int sm_i32x4 __attribute__((ext_vector_type(4)));
typedef float sm_f32x4 __attribute__((ext_vector_type(4)));

// grid (blocks per image, n); one thread = 4 consecutive channels of a position per pass (c % 4 == 0)
__global__ void __launch_bounds__(256) step_map_symbols_kernel(const float* __restrict__ y, const float* __restrict__ mu,
                                                               const unsigned short* __restrict__ tid0, long long hw, int c,
                                                               int mu_stride, const signed char* __restrict__ kmap,
                                                               const float* __restrict__ lut, int* __restrict__ symbols,
                                                               unsigned short* __restrict__ tid) {
  const int img = blockIdx.y, c4 = c >> 2;
  const long long nvec = hw * c4, base = (long long)img * hw * c;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < nvec; i += (long long)gridDim.x * blockDim.x) {
    const long long p = i / c4;
    const int ch = (int)(i - p * c4) << 2;
    const int k = map_index(kmap[(long long)img * hw + p]);
    const float inv = lut[kMapLut + k - kMapMin];
    const sm_f32x4 yv = *reinterpret_cast<const sm_f32x4*>(y + base + i * 4);
    const sm_f32x4 m = *reinterpret_cast<const sm_f32x4*>(mu + ((long long)img * hw + p) * mu_stride + ch);
    const ushort4 t = *reinterpret_cast<const ushort4*>(tid0 + base + i * 4);
    sm_i32x4 s;
#pragma unroll
    for (int e = 0; e < 4; ++e) s[e] = step_round(step_diff(yv[e], m[e]), inv);
    ushort4 o;
    o.x = (unsigned short)step_table_id(t.x, k);
    o.y = (unsigned short)step_table_id(t.y, k);
    o.z = (unsigned short)step_table_id(t.z, k);
    o.w = (unsigned short)step_table_id(t.w, k);
    *reinterpret_cast<sm_i32x4*>(symbols + base + i * 4) = s;
    *reinterpret_cast<ushort4*>(tid + base + i * 4) = o;
  }
}

// the decoder's half of step_map_symbols_kernel: it has the ids of the hyper-synthesis and no y
__global__ void __launch_bounds__(256) step_map_table_ids_kernel(const unsigned short* __restrict__ tid0, long long hw, int c,
                                                                 const signed char* __restrict__ kmap,
                                                                 unsigned short* __restrict__ tid) {
  const long long elems = hw * c, base = (long long)blockIdx.y * elems;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < elems; i += (long long)gridDim.x * blockDim.x) {
    const int k = map_index(kmap[(long long)blockIdx.y * hw + i / c]);
    tid[base + i] = (unsigned short)step_table_id(tid0[base + i], k);
  }
}

__global__ void __launch_bounds__(256) dequant_step_map_kernel(const int* __restrict__ symbols, const float* __restrict__ mu,
                                                               long long hw, int c, int mu_stride,
                                                               const signed char* __restrict__ kmap, const float* __restrict__ lut,
                                                               float* __restrict__ y_hat) {
  const int img = blockIdx.y, c4 = c >> 2;
  const long long nvec = hw * c4, base = (long long)img * hw * c;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < nvec; i += (long long)gridDim.x * blockDim.x) {
    const long long p = i / c4;
    const int ch = (int)(i - p * c4) << 2;
    const float st = lut[map_index(kmap[(long long)img * hw + p]) - kMapMin];
    const sm_i32x4 s = *reinterpret_cast<const sm_i32x4*>(symbols + base + i * 4);
    const sm_f32x4 m = *reinterpret_cast<const sm_f32x4*>(mu + ((long long)img * hw + p) * mu_stride + ch);
    sm_f32x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = step_value(s[e], m[e], st);
    *reinterpret_cast<sm_f32x4*>(y_hat + base + i * 4) = o;
  }
}

// grid (workgroups per image, n): no workgroup straddles an image.  A thread's unit is V elements of one position (V = 4: one
// 16-byte load of y and of mu, 8 bytes of ids; V = 1 where a pointer is not aligned for that), so it has ONE offset; (position,
// unit in the position) advance by the launch's stride as (dq, dr): no division in the loop.  nsteps <= kMapLadderMax candidate
// bases, uniform; their sums 64-bit per lane.
template <bool LDS, int V>
__global__ void __launch_bounds__(kMapLadderThreads) step_map_ladder_cost_kernel(
    const float* __restrict__ y, const float* __restrict__ mu, const unsigned short* __restrict__ tid0, long long hw, int c,
    int mu_stride, const signed char* __restrict__ offsets, const float* __restrict__ lut, const int* __restrict__ kbase, int nsteps,
    RansTables T, const unsigned* __restrict__ cost_q, int dq, int dr, unsigned long long* __restrict__ cost) {
  extern __shared__ unsigned char smem[];
  __shared__ unsigned long long partial[kMapLadderThreads / 64][kMapLadderMax];
  __shared__ float sinv[kMapLut];
  const uint2* meta = T.meta;
  const unsigned* cq = cost_q;
  if (threadIdx.x < kMapLut) sinv[threadIdx.x] = lut[kMapLut + threadIdx.x];
  if (LDS) {
    uint2* m = reinterpret_cast<uint2*>(smem);
    unsigned* q = reinterpret_cast<unsigned*>(smem + (size_t)T.ntables * sizeof(uint2));
    for (int i = threadIdx.x; i < T.ntables; i += kMapLadderThreads) m[i] = T.meta[i];
    for (int i = threadIdx.x; i < T.total; i += kMapLadderThreads) q[i] = cost_q[i];
    meta = m;
    cq = q;
  }
  __syncthreads();
  int kb[kMapLadderMax];
  unsigned long long sum[kMapLadderMax];
#pragma unroll
  for (int k = 0; k < kMapLadderMax; ++k) {
    kb[k] = k < nsteps ? min(max(kbase[k], -256), 256) : 0;  // beyond +-160 every int8 offset clips to the same end: same result,
                                                             // and base + offset cannot overflow
    sum[k] = 0ull;
  }
  const int img = blockIdx.y, cu = c / V;                    // units per position
  const long long nunit = hw * cu, base = (long long)img * hw * c;
  const long long stride = (long long)gridDim.x * kMapLadderThreads;
  const long long i0 = (long long)blockIdx.x * kMapLadderThreads + threadIdx.x;
  long long p = i0 / cu;
  int r = (int)(i0 - p * cu);
  for (long long i = i0; i < nunit; i += stride) {
    float d[V];
    unsigned t0[V];
    const float* yp = y + base + i * V;
    const float* mp = mu + ((long long)img * hw + p) * mu_stride + r * V;
    const unsigned short* tp = tid0 + base + i * V;
    const int off = offsets[(long long)img * hw + p];
    if (V == 4) {
      const sm_f32x4 yv = *reinterpret_cast<const sm_f32x4*>(yp);
      const sm_f32x4 mv = *reinterpret_cast<const sm_f32x4*>(mp);
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
    for (int k = 0; k < kMapLadderMax; ++k) {
      if (k < nsteps) {
        const int idx = map_index(kb[k] + off);
        const float inv = sinv[idx - kMapMin];
        unsigned part = 0u;                                  // <= 4 x 2^22: an entry of cost_q is below (16 + 16) x 65536
#pragma unroll
        for (int e = 0; e < V; ++e) {
          const uint2 m = meta[step_table_id(t0[e], idx)];
          bool esc;
          const int sym = rans_symbol(step_round(d[e], inv), m, esc);
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
  for (int k = 0; k < kMapLadderMax; ++k) {
    if (k < nsteps) {
      unsigned long long s = sum[k];
      for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o);
      if (lane == 0) partial[wave][k] = s;
    }
  }
  __syncthreads();
  if (threadIdx.x < nsteps) {
    unsigned long long s = 0ull;
    for (int w = 0; w < kMapLadderThreads / 64; ++w) s += partial[w][threadIdx.x];
    atomicAdd(&cost[(long long)img * nsteps + threadIdx.x], s);
  }
}

template <bool LDS, int V>
static int launch_map_ladder(dim3 grid, int lds, hipStream_t s, const float* y, const float* mu, const unsigned short* tid0,
                             long long hw, int c, int mu_stride, const signed char* offsets, const float* lut, const int* kbase,
                             int nsteps, const RansTables& T, const unsigned* cost_q, unsigned long long* cost) {
  if (LDS) SNTC_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(step_map_ladder_cost_kernel<LDS, V>), hipFuncAttributeMaxDynamicSharedMemorySize, lds));
  const long long stride = (long long)grid.x * kMapLadderThreads;
  const int cu = c / V;
  hipLaunchKernelGGL((step_map_ladder_cost_kernel<LDS, V>), grid, dim3(kMapLadderThreads), LDS ? lds : 0, s, y, mu, tid0, hw, c,
                     mu_stride, offsets, lut, kbase, nsteps, T, cost_q, (int)(stride / cu), (int)(stride % cu), cost);
  SNTC_HIP(hipGetLastError());
  return SNTC_OK;
}

static bool map_sizes_ok(int n, int64_t hw, int c, int mu_stride) {
  return n >= 1 && n <= 65535 && hw >= 1 && c >= 1 && c % 4 == 0 && mu_stride >= c && mu_stride % 4 == 0;
}

static bool map_aligned(const void* p, uintptr_t a) { return reinterpret_cast<uintptr_t>(p) % a == 0; }

static unsigned map_blocks(int64_t nvec) { return (unsigned)std::min<int64_t>(std::max<int64_t>((nvec + 1023) / 1024, 1), 1024); }

}  // namespace sntc

using namespace sntc;

extern "C" int sntc_step_map_symbols(const float* y, const float* mu, int n, int64_t hw, int c, int mu_stride, const uint16_t* base_ids,
                                     const int8_t* kmap, const float* lut, int32_t* symbols, uint16_t* table_ids, void* stream) {
  if (!y || !mu || !base_ids || !kmap || !lut || !symbols || !table_ids)
    return fail(SNTC_ERR_BAD_SHAPE, "sntc_step_map_symbols: null argument");
  if (!map_sizes_ok(n, hw, c, mu_stride))
    return fail(SNTC_ERR_BAD_SHAPE, "sntc_step_map_symbols: bad sizes (1 <= n <= 65535, c % 4 == 0, mu_stride >= c, mu_stride % 4 == 0)");
  if (!map_aligned(y, 16) || !map_aligned(mu, 16) || !map_aligned(symbols, 16) || !map_aligned(base_ids, 8) || !map_aligned(table_ids, 8) ||
      !map_aligned(lut, 4))
    return fail(SNTC_ERR_BAD_SHAPE, "sntc_step_map_symbols: y / mu / symbols must be 16-byte aligned, the id arrays 8-byte aligned");
  hipLaunchKernelGGL(step_map_symbols_kernel, dim3(map_blocks(hw * (c / 4)), n), dim3(256), 0, (hipStream_t)stream, y, mu, base_ids,
                     (long long)hw, c, mu_stride, reinterpret_cast<const signed char*>(kmap), lut, symbols, table_ids);
  SNTC_HIP(hipGetLastError());
  return SNTC_OK;
}

extern "C" int sntc_step_map_table_ids(const uint16_t* base_ids, int n, int64_t hw, int c, const int8_t* kmap, uint16_t* table_ids,
                                       void* stream) {
  if (!base_ids || !kmap || !table_ids) return fail(SNTC_ERR_BAD_SHAPE, "sntc_step_map_table_ids: null argument");
  if (n < 1 || n > 65535 || hw < 1 || c < 1) return fail(SNTC_ERR_BAD_SHAPE, "sntc_step_map_table_ids: bad sizes (1 <= n <= 65535)");
  hipLaunchKernelGGL(step_map_table_ids_kernel, dim3(map_blocks(hw * c / 4 + 1), n), dim3(256), 0, (hipStream_t)stream, base_ids,
                     (long long)hw, c, reinterpret_cast<const signed char*>(kmap), table_ids);
  SNTC_HIP(hipGetLastError());
  return SNTC_OK;
}

extern "C" int sntc_dequant_step_map(const int32_t* symbols, const float* mu, int n, int64_t hw, int c, int mu_stride,
                                     const int8_t* kmap, const float* lut, float* y_hat, void* stream) {
  if (!symbols || !mu || !kmap || !lut || !y_hat) return fail(SNTC_ERR_BAD_SHAPE, "sntc_dequant_step_map: null argument");
  if (!map_sizes_ok(n, hw, c, mu_stride))
    return fail(SNTC_ERR_BAD_SHAPE, "sntc_dequant_step_map: bad sizes (1 <= n <= 65535, c % 4 == 0, mu_stride >= c, mu_stride % 4 == 0)");
  if (!map_aligned(symbols, 16) || !map_aligned(mu, 16) || !map_aligned(y_hat, 16) || !map_aligned(lut, 4))
    return fail(SNTC_ERR_BAD_SHAPE, "sntc_dequant_step_map: symbols / mu / y_hat must be 16-byte aligned");
  hipLaunchKernelGGL(dequant_step_map_kernel, dim3(map_blocks(hw * (c / 4)), n), dim3(256), 0, (hipStream_t)stream, symbols, mu,
                     (long long)hw, c, mu_stride, reinterpret_cast<const signed char*>(kmap), lut, y_hat);
  SNTC_HIP(hipGetLastError());
  return SNTC_OK;
}

extern "C" int sntc_step_map_ladder_cost(const float* y, const float* mu, int n, int64_t hw, int c, int mu_stride,
                                         const uint16_t* base_ids, const int8_t* offsets, const float* lut, const int32_t* base,
                                         int nsteps, const uint32_t* meta, int ntables, int total_entries, const uint32_t* cost_q,
                                         uint64_t* cost, void* stream) {
  if (!y || !mu || !base_ids || !offsets || !lut || !base || !meta || !cost_q || !cost)
    return fail(SNTC_ERR_BAD_SHAPE, "sntc_step_map_ladder_cost: null argument");
  if (!map_sizes_ok(n, hw, c, mu_stride))
    return fail(SNTC_ERR_BAD_SHAPE, "sntc_step_map_ladder_cost: bad sizes (1 <= n <= 65535, c % 4 == 0, mu_stride >= c, mu_stride % 4 == 0)");
  if (nsteps < 1 || nsteps > kMapLadderMax) return fail(SNTC_ERR_BAD_SHAPE, "sntc_step_map_ladder_cost: 1 <= nsteps <= 16");
  if (ntables <= kLadderTop || total_entries < 1)
    return fail(SNTC_ERR_BAD_SHAPE, "sntc_step_map_ladder_cost: the table set must hold the 64 tables of the scale ladder");
  if (!map_aligned(y, 4) || !map_aligned(mu, 4) || !map_aligned(base_ids, 2) || !map_aligned(lut, 4) || !map_aligned(base, 4) ||
      !map_aligned(cost, 8))
    return fail(SNTC_ERR_BAD_SHAPE, "sntc_step_map_ladder_cost: misaligned argument");
  hipStream_t s = (hipStream_t)stream;
  if (int zrc = zero_async(cost, (size_t)n * nsteps * sizeof(uint64_t), s)) return zrc;
  const RansTables T{nullptr, reinterpret_cast<const uint2*>(meta), ntables, total_entries};   // the price replaces the cdf: never read
  const bool vec = map_aligned(y, 16) && map_aligned(mu, 16) && map_aligned(base_ids, 8);
  const long long nunit = (long long)hw * (c / (vec ? 4 : 1));
  const long long want = (nunit + kMapLadderThreads - 1) / kMapLadderThreads, most = std::max<long long>(1, kMapLadderGrid / n);
  const dim3 grid((unsigned)std::min(want, most), (unsigned)n);
  const long long tb = (long long)ntables * (long long)sizeof(uint2) + 4LL * total_entries;
  const bool lds = tb <= kMapLadderLdsLimit;
  unsigned long long* out = reinterpret_cast<unsigned long long*>(cost);
  const signed char* off = reinterpret_cast<const signed char*>(offsets);
  const int* kb = reinterpret_cast<const int*>(base);
  if (lds && vec) return launch_map_ladder<true, 4>(grid, (int)tb, s, y, mu, base_ids, hw, c, mu_stride, off, lut, kb, nsteps, T, cost_q, out);
  if (lds) return launch_map_ladder<true, 1>(grid, (int)tb, s, y, mu, base_ids, hw, c, mu_stride, off, lut, kb, nsteps, T, cost_q, out);
  if (vec) return launch_map_ladder<false, 4>(grid, 0, s, y, mu, base_ids, hw, c, mu_stride, off, lut, kb, nsteps, T, cost_q, out);
  return launch_map_ladder<false, 1>(grid, 0, s, y, mu, base_ids, hw, c, mu_stride, off, lut, kb, nsteps, T, cost_q, out);
}
