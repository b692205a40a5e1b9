// rdoq.hip -- rate-distortion optimised quantisation of the mean-scale hyperprior's latents ("RDOQ").  The
// reference rounds y - mu to the nearest integer (mshyper/models.py:273-279); sntc_step_symbols does the same at a step off the
// scale ladder.  Here the symbol of an element is the candidate with the smallest rate + weighted squared error, the rate being the
// exact integer price the coder's own table asks for it (cost_q, what sntc_rans_cost sums), the decision that of rdoq_rules.h:
//   d = step_diff(y, mu), u = step_scaled(d, inv), s0 = step_round(d, inv), t = step_table_id(t0, k), m = meta[t]
//   price(s) = cost_q[m.x + rans_symbol(s, m, esc)]
//   symbol = enable[image] ? rdoq_choose(u, s0, weight[channel], flags, price) : s0
// The table ids written are those of the step kernels: the files are ordinary wire format 3 / 5 / 7 and no decoder changes.
//
// One kernel body, template <bool MAP, bool LDS>: (k, inv) per image from shift / inv_step, or (MAP) per latent position from an
// int8 map and the step table `lut`, exactly as step_symbols_kernel (quant_step.hip) reads them, and its walk: grid (workgroups
// per image, n), one thread = 4 consecutive channels of a position per pass, 16-byte accesses.  The descriptors and cost_q are
// staged in dynamic LDS as step_ladder_cost_kernel stages them (64 normal tables: 62 KB, two workgroups of 16 waves per CU), so the
// launch has that kernel's shape -- 1024 threads, about kRdoqGrid workgroups, grid-stride -- and not step_symbols_kernel's many
// small workgroups: a workgroup pays its staging once.  Table sets beyond kRdoqLdsLimit are read from global memory (LDS =
// false).  A workgroup of an image that is not enabled stages nothing and looks nothing up: it writes step_symbols_kernel's bits.
// Per enabled element with s0 != 0 that is 2 - 3 dependent look-ups id -> descriptor -> price (one descriptor read, shared by
// the candidates) against 18 bytes of memory traffic: the bound expected is the ladder-cost kernel's, the dependent chain through
// LDS, not HBM (DESIGN.md 4.7 has the times: 0.91 x step_symbols + rans_cost on 11.8 M elements; no counter run has split them).
//
// changed[image] counts the elements written != s0: an integer per lane, wave shuffle, LDS across the waves, ONE atomicAdd per
// workgroup on an int zeroed by the launch -- the count does not depend on the launch geometry.
#include <algorithm>
#include "rans_common.h"
#include "rdoq_rules.h"
#include "step_rules.h"

namespace sntc {

constexpr int kRdoqThreads = 1024;
constexpr int kRdoqGrid = 512;                              // workgroups of a launch, about: two per CU
constexpr int kRdoqLdsLimit = kRansLdsTotal;                // descriptors + cost_q staged in LDS up to here

typedef int rq_i32x4 __attribute__((ext_vector_type(4)));
typedef float rq_f32x4 __attribute__((ext_vector_type(4)));

template <bool MAP, bool LDS>
__global__ void __launch_bounds__(kRdoqThreads) rdoq_symbols_kernel(
    const float* __restrict__ y, const float* __restrict__ mu, const unsigned short* __restrict__ tid0, long long hw, int c,
    int mu_stride, const float* __restrict__ inv_step, const int* __restrict__ shift, const signed char* __restrict__ kmap,
    const float* __restrict__ lut, const float* __restrict__ weight, const int* __restrict__ enable, int flags, RansTables T,
    const unsigned* __restrict__ cost_q, int* __restrict__ symbols, unsigned short* __restrict__ tid, int* __restrict__ changed) {
  extern __shared__ unsigned char smem[];
  __shared__ int partial[kRdoqThreads / 64];
  const int img = blockIdx.y, c4 = c >> 2;
  const bool on = enable[img] != 0;                          // uniform in the workgroup
  const uint2* meta = T.meta;
  const unsigned* cq = cost_q;
  if constexpr (LDS) {
    if (on) {
      uint2* m = reinterpret_cast<uint2*>(smem);
      unsigned* q = reinterpret_cast<unsigned*>(smem + (size_t)T.ntables * sizeof(uint2));
      for (int i = threadIdx.x; i < T.ntables; i += kRdoqThreads) m[i] = T.meta[i];
      for (int i = threadIdx.x; i < T.total; i += kRdoqThreads) q[i] = cost_q[i];
      meta = m;
      cq = q;
    }
    __syncthreads();
  }
  float inv = 1.0f;
  int k = 0;
  if constexpr (!MAP) {
    inv = inv_step[img];
    k = shift[img];
  }
  int count = 0;
  const long long nvec = hw * c4, base = (long long)img * hw * c;
  for (long long i = blockIdx.x * (long long)kRdoqThreads + threadIdx.x; i < nvec; i += (long long)gridDim.x * kRdoqThreads) {
    const long long p = i / c4;
    const int ch = (int)(i - p * c4) << 2;
    if constexpr (MAP) {
      k = map_index(kmap[(long long)img * hw + p]);
      inv = lut[kMapLut + k - kMapMin];
    }
    const rq_f32x4 m = *reinterpret_cast<const rq_f32x4*>(mu + ((long long)img * hw + p) * mu_stride + ch);
    const ushort4 t = *reinterpret_cast<const ushort4*>(tid0 + base + i * 4);
    const rq_f32x4 yv = *reinterpret_cast<const rq_f32x4*>(y + base + i * 4);
    const unsigned ts[4] = {step_table_id(t.x, k), step_table_id(t.y, k), step_table_id(t.z, k), step_table_id(t.w, k)};
    rq_i32x4 s;
    if (on) {
      const rq_f32x4 w = *reinterpret_cast<const rq_f32x4*>(weight + ch);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float d = step_diff(yv[e], m[e]);
        const int s0 = step_round(d, inv);
        int pick = s0;
        if (s0 != 0) {
          const uint2 ds = meta[ts[e]];
          pick = rdoq_choose(step_scaled(d, inv), s0, w[e], flags, [&](int v) -> unsigned {
            bool esc;
            return cq[ds.x + rans_symbol(v, ds, esc)];
          });
        }
        count += pick != s0;
        s[e] = pick;
      }
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) s[e] = step_round(step_diff(yv[e], m[e]), inv);
    }
    ushort4 o;
    o.x = (unsigned short)ts[0];
    o.y = (unsigned short)ts[1];
    o.z = (unsigned short)ts[2];
    o.w = (unsigned short)ts[3];
    *reinterpret_cast<rq_i32x4*>(symbols + base + i * 4) = s;
    *reinterpret_cast<ushort4*>(tid + base + i * 4) = o;
  }
  if (changed == nullptr || !on) return;                     // uniform: nothing changes where the image is not enabled
  for (int off = 32; off > 0; off >>= 1) count += __shfl_down(count, off);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) partial[wave] = count;
  __syncthreads();
  if (threadIdx.x == 0) {
    int sum = 0;
    for (int w = 0; w < kRdoqThreads / 64; ++w) sum += partial[w];
    if (sum) atomicAdd(&changed[img], sum);
  }
}

static bool aligned(const void* p, uintptr_t a) { return reinterpret_cast<uintptr_t>(p) % a == 0; }

template <bool MAP, bool LDS>
static int launch_rdoq_instance(int lds, hipStream_t s, const float* y, const float* mu, const unsigned short* tid0, int n, long long hw,
                                int c, int mu_stride, const float* inv_step, const int* shift, const signed char* kmap, const float* lut,
                                const float* weight, const int* enable, int flags, const RansTables& T, const unsigned* cost_q,
                                int* symbols, unsigned short* tid, int* changed) {
  if (LDS) SNTC_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(rdoq_symbols_kernel<MAP, LDS>), hipFuncAttributeMaxDynamicSharedMemorySize, lds));
  const long long nvec = hw * (c / 4);
  const long long want = (nvec + kRdoqThreads - 1) / kRdoqThreads, most = std::max<long long>(1, kRdoqGrid / n);
  hipLaunchKernelGGL((rdoq_symbols_kernel<MAP, LDS>), dim3((unsigned)std::min(want, most), (unsigned)n), dim3(kRdoqThreads), LDS ? lds : 0, s,
                     y, mu, tid0, hw, c, mu_stride, inv_step, shift, kmap, lut, weight, enable, flags, T, cost_q, symbols, tid, changed);
  SNTC_HIP(hipGetLastError());
  return SNTC_OK;
}

// inv_step / shift (per image) or kmap / lut (MAP), the others null
template <bool MAP>
static int launch_rdoq(const char* who, const float* y, const float* mu, int n, int64_t hw, int c, int mu_stride, const uint16_t* base_ids,
                       const float* inv_step, const int32_t* shift, const int8_t* kmap, const float* lut, const float* weight,
                       const int32_t* enable, int flags, const uint32_t* meta, int ntables, int total_entries, const uint32_t* cost_q,
                       int32_t* symbols, uint16_t* table_ids, int32_t* changed, hipStream_t s) {
  const std::string name(who);
  if (!y || !mu || !base_ids || (MAP ? !kmap || !lut : !inv_step || !shift) || !weight || !enable || !meta || !cost_q || !symbols ||
      !table_ids)
    return fail(SNTC_ERR_BAD_SHAPE, name + ": null argument");
  if (!(n >= 1 && n <= 65535 && hw >= 1 && c >= 1 && c % 4 == 0 && mu_stride >= c && mu_stride % 4 == 0))
    return fail(SNTC_ERR_BAD_SHAPE, name + ": bad sizes (1 <= n <= 65535, c % 4 == 0, mu_stride >= c, mu_stride % 4 == 0)");
  if (ntables <= kLadderTop || total_entries < 1)
    return fail(SNTC_ERR_BAD_SHAPE, name + ": the table set must hold the 64 tables of the scale ladder");
  if (!aligned(y, 16) || !aligned(mu, 16) || !aligned(symbols, 16) || !aligned(weight, 16) || !aligned(base_ids, 8) ||
      !aligned(table_ids, 8) || !aligned(enable, 4) || !aligned(changed, 4) || (MAP && !aligned(lut, 4)))
    return fail(SNTC_ERR_BAD_SHAPE, name + ": y / mu / symbols / weight must be 16-byte aligned, the id arrays 8-byte aligned");
  if (changed)
    if (int zrc = zero_async(changed, (size_t)n * sizeof(int32_t), s)) return zrc;
  const RansTables T{nullptr, reinterpret_cast<const uint2*>(meta), ntables, total_entries};   // the price replaces the cdf: never read
  const long long tb = (long long)ntables * (long long)sizeof(uint2) + 4LL * total_entries;
  const auto launch = tb <= kRdoqLdsLimit ? launch_rdoq_instance<MAP, true> : launch_rdoq_instance<MAP, false>;
  return launch(tb <= kRdoqLdsLimit ? (int)tb : 0, s, y, mu, base_ids, n, hw, c, mu_stride, inv_step, reinterpret_cast<const int*>(shift),
                reinterpret_cast<const signed char*>(kmap), lut, weight, reinterpret_cast<const int*>(enable), flags, T, cost_q,
                reinterpret_cast<int*>(symbols), table_ids, reinterpret_cast<int*>(changed));
}

}  // namespace sntc

using namespace sntc;

extern "C" int sntc_rdoq_symbols(const float* y, const float* mu, int n, int64_t hw, int c, int mu_stride, const uint16_t* base_ids,
                                 const float* inv_step, const int32_t* shift, const float* weight, const int32_t* enable, int flags,
                                 const uint32_t* meta, int ntables, int total_entries, const uint32_t* cost_q, int32_t* symbols,
                                 uint16_t* table_ids, int32_t* changed, void* stream) {
  return launch_rdoq<false>("sntc_rdoq_symbols", y, mu, n, hw, c, mu_stride, base_ids, inv_step, shift, nullptr, nullptr, weight, enable,
                            flags, meta, ntables, total_entries, cost_q, symbols, table_ids, changed, (hipStream_t)stream);
}

extern "C" int sntc_rdoq_map_symbols(const float* y, const float* mu, int n, int64_t hw, int c, int mu_stride, const uint16_t* base_ids,
                                     const int8_t* kmap, const float* lut, const float* weight, const int32_t* enable, int flags,
                                     const uint32_t* meta, int ntables, int total_entries, const uint32_t* cost_q, int32_t* symbols,
                                     uint16_t* table_ids, int32_t* changed, void* stream) {
  return launch_rdoq<true>("sntc_rdoq_map_symbols", y, mu, n, hw, c, mu_stride, base_ids, nullptr, nullptr, kmap, lut, weight, enable,
                           flags, meta, ntables, total_entries, cost_q, symbols, table_ids, changed, (hipStream_t)stream);
}
