// rans_cost.hip -- what a set of integers costs in the bitstream of rans.hip, without coding them: the sum, per image, of
// cost_q[symbol] over the image's elements, cost_q = (16 - log2 frequency) in units of 2^-16 bit from the integer tables the
// coder itself uses (ESCAPE entries carry the 16 raw bits of the value on top).  The symbol of a value is rans_symbol(), the
// encoders' own.  What the file pays beyond this sum is the flushed lane states and the renormalisation slack of the 32-bit
// states.
//
// A stream, not a lone wave: 6 bytes in per element (int32 value, uint16 table id), nothing out but one 64-bit atomic per
// workgroup.  Grid = (workgroups per image, images): no workgroup straddles an image.  The descriptors and cost_q sit in LDS
// where they fit (64 normal tables: 62 KB, two workgroups per CU), else they are read from global memory, as the coder reads
// its tables.  Every sum is an integer (64 bits per lane, wave shuffle, LDS across the waves, atomicAdd on unsigned long long),
// so the result does not depend on the launch geometry or on the order the atomics arrive in.
#include <algorithm>
#include "rans_common.h"

namespace sntc {

constexpr int kCostThreads = 1024;                          // 16 waves; two workgroups of them per CU with the tables in LDS
constexpr int kCostVec = 4;                                 // elements per lane and load where the image size allows (16 + 8 bytes)
constexpr int kCostGrid = 512;                              // workgroups of a launch, about: two per CU
constexpr int kCostLdsLimit = kRansLdsTotal;                // descriptors + cost_q staged in LDS up to here

static inline long long rans_cost_table_bytes(int ntables, int total) { return (long long)ntables * (long long)sizeof(uint2) + 4LL * total; }

template <bool LDS, int V>
__global__ void __launch_bounds__(kCostThreads) rans_cost_kernel(const int* __restrict__ values, const unsigned short* __restrict__ tid,
                                                                 long long E, RansTables T, const unsigned* __restrict__ cost_q,
                                                                 unsigned long long* __restrict__ cost) {
  extern __shared__ unsigned char smem[];
  __shared__ unsigned long long partial[kCostThreads / 64];
  const uint2* meta = T.meta;
  const unsigned* cq = cost_q;
  if (LDS) {
    uint2* m = reinterpret_cast<uint2*>(smem);
    unsigned* c = reinterpret_cast<unsigned*>(smem + (size_t)T.ntables * sizeof(uint2));
    for (int i = threadIdx.x; i < T.ntables; i += kCostThreads) m[i] = T.meta[i];
    for (int i = threadIdx.x; i < T.total; i += kCostThreads) c[i] = cost_q[i];
    __syncthreads();
    meta = m;
    cq = c;
  }
  auto price = [&](int v, unsigned t) -> unsigned {
    const uint2 m = meta[t];
    bool esc;
    const int sym = rans_symbol(v, m, esc);
    return cq[m.x + sym];
  };
  const long long base = (long long)blockIdx.y * E;          // this image's first element
  const long long stride = (long long)gridDim.x * kCostThreads;
  unsigned long long sum = 0ull;
  if (V == 4) {                                              // E % 4 == 0 and both arrays aligned (host): whole vectors only
    const int4* v4 = reinterpret_cast<const int4*>(values + base);
    const ushort4* t4 = reinterpret_cast<const ushort4*>(tid + base);
    const long long nvec = E / 4;
#pragma unroll 2
    for (long long i = (long long)blockIdx.x * kCostThreads + threadIdx.x; i < nvec; i += stride) {
      const int4 v = v4[i];
      const ushort4 t = t4[i];
      sum += (unsigned long long)price(v.x, t.x) + price(v.y, t.y) + price(v.z, t.z) + price(v.w, t.w);
    }
  } else {
#pragma unroll 4
    for (long long i = (long long)blockIdx.x * kCostThreads + threadIdx.x; i < E; i += stride) sum += price(values[base + i], tid[base + i]);
  }
  for (int off = 32; off > 0; off >>= 1) sum += __shfl_down(sum, off);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) partial[wave] = sum;
  __syncthreads();
  if (wave == 0) {
    sum = lane < kCostThreads / 64 ? partial[lane] : 0ull;
    for (int off = kCostThreads / 128; off > 0; off >>= 1) sum += __shfl_down(sum, off);
    if (lane == 0) atomicAdd(&cost[blockIdx.y], sum);
  }
}

template <bool LDS, int V>
static int launch_cost(dim3 grid, int lds, hipStream_t s, const int* values, const unsigned short* tid, long long E, const RansTables& T,
                        const unsigned* cost_q, unsigned long long* cost) {
  if (LDS) SNTC_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(rans_cost_kernel<LDS, V>), hipFuncAttributeMaxDynamicSharedMemorySize, lds));
  hipLaunchKernelGGL((rans_cost_kernel<LDS, V>), grid, dim3(kCostThreads), LDS ? lds : 0, s, values, tid, E, T, cost_q, cost);
  SNTC_HIP(hipGetLastError());
  return SNTC_OK;
}

}  // namespace sntc

using namespace sntc;

extern "C" int sntc_rans_cost(const int32_t* values, const uint16_t* table_ids, int nimages, int64_t elems_per_image,
                              const uint32_t* meta, int ntables, int total_entries, const uint32_t* cost_q, uint64_t* cost, void* stream) {
  if (!values || !table_ids || !meta || !cost_q || !cost) return fail(SNTC_ERR_BAD_SHAPE, "sntc_rans_cost: null argument");
  if (nimages < 1 || nimages > 65535 || elems_per_image < 1 || ntables < 1 || total_entries < 1)
    return fail(SNTC_ERR_BAD_SHAPE, "sntc_rans_cost: bad sizes (1 <= nimages <= 65535)");
  hipStream_t s = (hipStream_t)stream;
  if (int zrc = zero_async(cost, (size_t)nimages * sizeof(uint64_t), s)) return zrc;
  const RansTables T{nullptr, reinterpret_cast<const uint2*>(meta), ntables, total_entries};   // the price replaces the cdf: never read
  const long long E = elems_per_image;
  const bool vec = E % kCostVec == 0 && reinterpret_cast<uintptr_t>(values) % 16 == 0 && reinterpret_cast<uintptr_t>(table_ids) % 8 == 0;
  const long long span = (long long)kCostThreads * (vec ? kCostVec : 1);      // elements one workgroup takes per pass
  const long long want = (E + span - 1) / span, most = std::max<long long>(1, kCostGrid / nimages);   // want >= 1: E >= 1
  const dim3 grid((unsigned)std::min(want, most), (unsigned)nimages);
  const long long tb = rans_cost_table_bytes(ntables, total_entries);
  const bool lds = tb <= kCostLdsLimit;
  unsigned long long* out = reinterpret_cast<unsigned long long*>(cost);
  if (lds && vec) return launch_cost<true, 4>(grid, (int)tb, s, values, table_ids, E, T, cost_q, out);
  if (lds) return launch_cost<true, 1>(grid, (int)tb, s, values, table_ids, E, T, cost_q, out);
  if (vec) return launch_cost<false, 4>(grid, 0, s, values, table_ids, E, T, cost_q, out);
  return launch_cost<false, 1>(grid, 0, s, values, table_ids, E, T, cost_q, out);
}
