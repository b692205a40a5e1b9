// quant_step.hip -- the latents of the mean-scale hyperprior quantised with a step off the scale ladder (DESIGN.md 4.7,
// "variable rate", "quality target").  The 64 coding tables sit on sigma_i = 0.11 r^i, r = exp(kScaleFactor): a symbol
// round((y - mu) / r^k) of an element whose table would be i is distributed as table i - k describes, so the tables, the coder and
// the decoder serve every step k of the ladder unchanged.  Three rules, one device function each (step_rules.h: SGA at a step,
// sga.hip, samples and dequantises with the same functions), applied by every kernel here:
//   symbol    s = (int)rintf((y - mu) * inv_step)            step_round(step_diff): float32 subtract, then float32 multiply
//   table id  t = clamp(t0 - k, 0, 63)                       step_table_id; t0 = sntc_scale_table_ids; off the ladder's ends the
//                                                            end table stays
//   value     y_hat = fmaf(step, (float)s, mu)               step_value
// At k = 0 (step = inv_step = 1.0f) they are the symbols of sntc_entropy_scale_normal, the ids of sntc_scale_table_ids and the
// values of sntc_dequant_mean, bit for bit.
//
// Two sources of the triple (k, step, inv_step), one kernel body for both (template <bool MAP>, as sga.hip has it):
//   per image     the host's arrays shift / step / inv_step, one entry per image (or per candidate of a ladder): uniform, read
//                 ONCE before the loop.
//   per position  (MAP; region-of-interest coding, wire format 7) all c channels of a latent position share one index k in
//                 [-32, 32] from an int8 map [n][hw].  step(k) / inv_step(k) are never computed here: the host uploads ONE table
//                 `lut`, float32 [2][65], row 0 = step, row 1 = inv_step, indexed by k + 32 (entropy_coding.step_size: float64,
//                 rounded once).  Every kernel clamps the index it reads into [-32, 32] first (map_index), so a stray byte in a
//                 map can never read outside the table; the host validates the maps anyway.  With a constant map these are the
//                 symbols, ids, values and costs of the per-image instances at that index, bit for bit.
//
// step_ladder_cost_kernel is rans_cost_kernel (rans_cost.hip) with the symbols formed on the fly for up to kLadderMax candidate
// steps at once: y, mu and the base ids are read ONCE (10 bytes per element), every candidate's symbol is priced from the tables
// in LDS, and the sums stay integers from the lane to the atomic -- the result does not depend on the launch geometry.  Per
// element that is 2 K LDS reads (descriptor, price) against 10 bytes from memory: the launch is not HBM-bound (measured 0.76 TB/s
// at K = 16 on 8.8 M elements, 2.7 look-ups per clock and CU); by bank arithmetic neither LDS nor VALU issue is saturated, it is
// the dependent chain id -> descriptor -> symbol -> price across both pipes; no counter run has split the two.
// MAP: candidate j's index at position p is map_index(base[j] + offsets[p]); a thread's unit is V channels of ONE position, so it
// reads one offset per unit and, per candidate, one inverse step from the 65 floats staged in LDS.
//
// step_ladder_dequant_kernel is the distortion side of the same ladder: what each candidate DECODES to.  The reference quantises
// y - mu with step 1 and decodes y_hat = round(y - mu) + mu (mshyper/models.py:273-279, one decode per evaluation); here, per
// element and candidate j,
//   s     = step_round(step_diff(y, mu), inv_step[j])        never clamped: the symbol coded_cost decodes, not the file's
//   y_hat = step_value(s, mu, step[j])                       16-bit escape
// written to y_hat[j][image][position][channel]: candidate j is a contiguous batch of n latents the decoder takes as it is, so
// the nsteps candidates of n images are ONE decoder batch of nsteps n.  Candidate plane j equals sntc_dequant_step of
// sntc_step_symbols at that step (sntc_dequant_step_map of sntc_step_map_symbols with MAP), bit for bit.  It is a store stream:
// y and mu are read once per launch (8 bytes per element), every load feeds nsteps stores (4 nsteps bytes per element): with 16
// candidates 64 bytes out per 8 in, the roof is HBM write bandwidth.  No atomics, no LDS; the MAP instances read the 65-entry
// step table through the vector cache.
//
// Requantisation (REQ; transcoding a file to a coarser step without pixels, DESIGN.md 4.7 "transcode"): the source is not y but
// the integers s0 a file holds at the indexes k0 of its own grid (a source map int8 [n][hw], clamped with map_index like every
// map).  The difference the symbol rule rounds is then that of the value the decoder would feed the synthesis,
//   d = step_diff(step_value(s0, mu, step[k0]), mu)          y_hat0 rounded to float32 once, as sntc_dequant_step_map stores it
// and everything after d is the MAP instance unchanged: step_symbols_kernel<true, true> writes step_round(d, inv_step[k1]) and
// step_table_id(base, k1) at k1 = a destination map's index, step_ladder_cost_kernel<true, ., ., true> prices candidate j at
// k1 = map_index(k0 + shift[j]).  They equal the MAP entry points on the stored sntc_dequant_step_map values, bit for bit; no
// y_hat tensor is written.
#include <algorithm>
#include "rans_common.h"
#include "step_rules.h"

namespace sntc {

// kMapMin / kMapMax / kMapLut and map_index: step_rules.h (the SGA map kernels of sga.hip read the same table)
constexpr int kLadderMax = 16;                              // candidates of one ladder launch (their sums / steps live in registers)
constexpr int kLadderThreads = 1024;
constexpr int kLadderGrid = 512;                            // workgroups of a cost launch, about
constexpr int kLadderLdsLimit = kRansLdsTotal;              // descriptors + cost_q staged in LDS up to here
constexpr int kDequantLadderThreads = 256;
constexpr int kDequantLadderGrid = 2048;                    // workgroups of a dequant launch, about: 8 per CU, grid-stride beyond

typedef int qs_i32x4 __attribute__((ext_vector_type(4)));
typedef float qs_f32x4 __attribute__((ext_vector_type(4)));

// grid (blocks per image, n); one thread = 4 consecutive channels of a position per pass (c % 4 == 0)
// REQ (with MAP): `src` holds a file's symbols (int32) in place of y, `src_map` the indexes they were quantised at; kmap is the
// destination.
template <bool MAP, bool REQ = false>
__global__ void __launch_bounds__(256) step_symbols_kernel(const void* __restrict__ src, const float* __restrict__ mu,
                                                           const unsigned short* __restrict__ tid0, long long hw, int c, int mu_stride,
                                                           const float* __restrict__ inv_step, const int* __restrict__ shift,
                                                           const signed char* __restrict__ src_map,
                                                           const signed char* __restrict__ kmap, const float* __restrict__ lut,
                                                           int* __restrict__ symbols, unsigned short* __restrict__ tid) {
  static_assert(MAP || !REQ, "requantisation reads its grids from maps");
  const float* y = static_cast<const float*>(src);
  const int* s0 = static_cast<const int*>(src);
  const int img = blockIdx.y, c4 = c >> 2;
  float inv = 1.0f, st0 = 1.0f;
  int k = 0;
  if constexpr (!MAP) { inv = inv_step[img]; k = shift[img]; }
  const long long nvec = hw * c4, base = (long long)img * hw * c;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < nvec; i += (long long)gridDim.x * blockDim.x) {
    const long long p = i / c4;
    const int ch = (int)(i - p * c4) << 2;
    if constexpr (MAP) {
      k = map_index(kmap[(long long)img * hw + p]);
      inv = lut[kMapLut + k - kMapMin];
      if constexpr (REQ) st0 = lut[map_index(src_map[(long long)img * hw + p]) - kMapMin];
    }
    const qs_f32x4 m = *reinterpret_cast<const qs_f32x4*>(mu + ((long long)img * hw + p) * mu_stride + ch);
    const ushort4 t = *reinterpret_cast<const ushort4*>(tid0 + base + i * 4);
    qs_f32x4 yv;
    if constexpr (REQ) {
      const qs_i32x4 sv = *reinterpret_cast<const qs_i32x4*>(s0 + base + i * 4);
#pragma unroll
      for (int e = 0; e < 4; ++e) yv[e] = step_value(sv[e], m[e], st0);
    } else {
      yv = *reinterpret_cast<const qs_f32x4*>(y + base + i * 4);
    }
    qs_i32x4 s;
#pragma unroll
    for (int e = 0; e < 4; ++e) s[e] = step_round(step_diff(yv[e], m[e]), inv);
    ushort4 o;
    o.x = (unsigned short)step_table_id(t.x, k);
    o.y = (unsigned short)step_table_id(t.y, k);
    o.z = (unsigned short)step_table_id(t.z, k);
    o.w = (unsigned short)step_table_id(t.w, k);
    *reinterpret_cast<qs_i32x4*>(symbols + base + i * 4) = s;
    *reinterpret_cast<ushort4*>(tid + base + i * 4) = o;
  }
}

// the decoder's half of step_symbols_kernel: it has the ids of the hyper-synthesis and no y.  Per image the caller's elements
// are hw with c = 1.
template <bool MAP>
__global__ void __launch_bounds__(256) step_table_ids_kernel(const unsigned short* __restrict__ tid0, long long hw, int c,
                                                             const int* __restrict__ shift, const signed char* __restrict__ kmap,
                                                             unsigned short* __restrict__ tid) {
  int k = 0;
  if constexpr (!MAP) k = shift[blockIdx.y];
  const long long elems = hw * c, base = (long long)blockIdx.y * elems;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < elems; i += (long long)gridDim.x * blockDim.x) {
    if constexpr (MAP) k = map_index(kmap[(long long)blockIdx.y * hw + i / c]);
    tid[base + i] = (unsigned short)step_table_id(tid0[base + i], k);
  }
}

template <bool MAP>
__global__ void __launch_bounds__(256) dequant_step_kernel(const int* __restrict__ symbols, const float* __restrict__ mu, long long hw,
                                                           int c, int mu_stride, const float* __restrict__ step,
                                                           const signed char* __restrict__ kmap, const float* __restrict__ lut,
                                                           float* __restrict__ y_hat) {
  const int img = blockIdx.y, c4 = c >> 2;
  float st = 1.0f;
  if constexpr (!MAP) st = step[img];
  const long long nvec = hw * c4, base = (long long)img * hw * c;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < nvec; i += (long long)gridDim.x * blockDim.x) {
    const long long p = i / c4;
    const int ch = (int)(i - p * c4) << 2;
    if constexpr (MAP) st = lut[map_index(kmap[(long long)img * hw + p]) - kMapMin];
    const qs_i32x4 s = *reinterpret_cast<const qs_i32x4*>(symbols + base + i * 4);
    const qs_f32x4 m = *reinterpret_cast<const qs_f32x4*>(mu + ((long long)img * hw + p) * mu_stride + ch);
    qs_f32x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = step_value(s[e], m[e], st);
    *reinterpret_cast<qs_f32x4*>(y_hat + base + i * 4) = o;
  }
}

// The walk of the two ladder kernels.  Grid (workgroups per image, n): no workgroup straddles an image.  A thread's unit is V
// elements of one position (V = 4: 16-byte accesses; V = 1 where a pointer is not aligned for that), unit r of the position's cu;
// the launch's stride in units, split by the host as dq positions and dr units (unit_grid), advances it: no division in the loop.
__device__ __forceinline__ void next_unit(long long& p, int& r, int cu, int dq, int dr) {
  p += dq;
  r += dr;
  if (r >= cu) {
    r -= cu;
    ++p;
  }
}

// nsteps <= kLadderMax candidates, uniform, their sums 64-bit per lane: inv_step / shift [nsteps], or (MAP) the bases kbase
// [nsteps] added to the position's byte of offsets [n][hw].
// REQ (with MAP): `src` holds a file's symbols (int32) in place of y, `offsets` the indexes k0 they were quantised at (the source
// map) and kbase the candidates' shifts; the step of k0 comes from row 0 of lut, staged beside the inverse steps.
template <bool MAP, bool LDS, int V, bool REQ = false>
__global__ void __launch_bounds__(kLadderThreads) step_ladder_cost_kernel(
    const void* __restrict__ src, const float* __restrict__ mu, const unsigned short* __restrict__ tid0, long long hw, int c,
    int mu_stride, const float* __restrict__ inv_step, const int* __restrict__ shift, const signed char* __restrict__ offsets,
    const float* __restrict__ lut, const int* __restrict__ kbase, int nsteps, RansTables T, const unsigned* __restrict__ cost_q, int dq,
    int dr, unsigned long long* __restrict__ cost) {
  extern __shared__ unsigned char smem[];
  __shared__ unsigned long long partial[kLadderThreads / 64][kLadderMax];
  const uint2* meta = T.meta;
  const unsigned* cq = cost_q;
  static_assert(MAP || !REQ, "requantisation reads its grids from maps");
  const float* y = static_cast<const float*>(src);
  const int* s0 = static_cast<const int*>(src);
  const float* sinv = nullptr;
  const float* sstep = nullptr;
  if constexpr (MAP) {
    __shared__ float row[kMapLut];
    if (threadIdx.x < kMapLut) row[threadIdx.x] = lut[kMapLut + threadIdx.x];
    sinv = row;
  }
  if constexpr (REQ) {
    __shared__ float row0[kMapLut];
    if (threadIdx.x < kMapLut) row0[threadIdx.x] = lut[threadIdx.x];
    sstep = row0;
  }
  if constexpr (LDS) {
    uint2* m = reinterpret_cast<uint2*>(smem);
    unsigned* q = reinterpret_cast<unsigned*>(smem + (size_t)T.ntables * sizeof(uint2));
    for (int i = threadIdx.x; i < T.ntables; i += kLadderThreads) m[i] = T.meta[i];
    for (int i = threadIdx.x; i < T.total; i += kLadderThreads) q[i] = cost_q[i];
    meta = m;
    cq = q;
  }
  if constexpr (LDS || MAP) __syncthreads();
  float inv[kLadderMax];
  int sh[kLadderMax], kb[kLadderMax];
  unsigned long long sum[kLadderMax];
#pragma unroll
  for (int k = 0; k < kLadderMax; ++k) {
    if constexpr (MAP) {
      kb[k] = k < nsteps ? min(max(kbase[k], -256), 256) : 0;  // beyond +-160 every int8 offset clips to the same end: same result,
                                                               // and base + offset cannot overflow
    } else {
      inv[k] = k < nsteps ? inv_step[k] : 0.0f;
      sh[k] = k < nsteps ? shift[k] : 0;
    }
    sum[k] = 0ull;
  }
  const int img = blockIdx.y, cu = c / V;                    // units per position
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
    int off = 0;
    if constexpr (MAP) off = offsets[(long long)img * hw + p];
    float st0 = 1.0f;
    if constexpr (REQ) {
      off = map_index(off);                                  // k0: the index the file's symbols were quantised at
      st0 = sstep[off - kMapMin];
    }
    if constexpr (V == 4) {
      const qs_f32x4 mv = *reinterpret_cast<const qs_f32x4*>(mp);
      qs_f32x4 yv;
      if constexpr (REQ) {
        const qs_i32x4 sv = *reinterpret_cast<const qs_i32x4*>(s0 + base + i * V);
#pragma unroll
        for (int e = 0; e < V; ++e) yv[e] = step_value(sv[e], mv[e], st0);
      } else {
        yv = *reinterpret_cast<const qs_f32x4*>(yp);
      }
      const ushort4 tv = *reinterpret_cast<const ushort4*>(tp);
      const unsigned short ts[4] = {tv.x, tv.y, tv.z, tv.w};
#pragma unroll
      for (int e = 0; e < V; ++e) {
        d[e] = step_diff(yv[e], mv[e]);
        t0[e] = ts[e];
      }
    } else {
      const float m0 = mp[0];
      float y0;
      if constexpr (REQ) y0 = step_value(s0[base + i], m0, st0);
      else y0 = yp[0];
      d[0] = step_diff(y0, m0);
      t0[0] = tp[0];
    }
#pragma unroll
    for (int k = 0; k < kLadderMax; ++k) {
      if (k < nsteps) {
        int idx;
        float iv;
        if constexpr (MAP) {
          idx = map_index(kb[k] + off);
          iv = sinv[idx - kMapMin];
        } else {
          idx = sh[k];
          iv = inv[k];
        }
        unsigned part = 0u;                                  // <= 4 x 2^22: an entry of cost_q is below (16 + 16) x 65536
#pragma unroll
        for (int e = 0; e < V; ++e) {
          const uint2 m = meta[step_table_id(t0[e], idx)];
          bool esc;
          const int sym = rans_symbol(step_round(d[e], iv), m, esc);
          part += cq[m.x + sym];
        }
        sum[k] += part;
      }
    }
    next_unit(p, r, cu, dq, dr);
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < kLadderMax; ++k) {
    if (k < nsteps) {
      unsigned long long s = sum[k];
      for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o);
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

// The same candidates (inv_step / step [nsteps], or with MAP kbase / offsets / lut), each one's values to its own plane of y_hat.
template <bool MAP, int V>
__global__ void __launch_bounds__(kDequantLadderThreads) step_ladder_dequant_kernel(
    const float* __restrict__ y, const float* __restrict__ mu, long long hw, int c, int mu_stride, const float* __restrict__ inv_step,
    const float* __restrict__ step, const signed char* __restrict__ offsets, const float* __restrict__ lut,
    const int* __restrict__ kbase, int nsteps, int dq, int dr, float* __restrict__ y_hat) {
  float inv[kLadderMax], st[kLadderMax];
  int kb[kLadderMax];
#pragma unroll
  for (int k = 0; k < kLadderMax; ++k) {
    if constexpr (MAP) {
      kb[k] = k < nsteps ? min(max(kbase[k], -256), 256) : 0;  // as in the cost kernel
    } else {
      inv[k] = k < nsteps ? inv_step[k] : 0.0f;
      st[k] = k < nsteps ? step[k] : 0.0f;
    }
  }
  const int img = blockIdx.y, cu = c / V;                    // units per position
  const long long nunit = hw * cu, base = (long long)img * hw * c, plane = (long long)gridDim.y * hw * c;
  const long long stride = (long long)gridDim.x * kDequantLadderThreads;
  const long long i0 = (long long)blockIdx.x * kDequantLadderThreads + threadIdx.x;
  long long p = i0 / cu;
  int r = (int)(i0 - p * cu);
  for (long long i = i0; i < nunit; i += stride) {
    float d[V], m[V];
    const float* yp = y + base + i * V;
    const float* mp = mu + ((long long)img * hw + p) * mu_stride + r * V;
    if constexpr (V == 4) {
      const qs_f32x4 yv = *reinterpret_cast<const qs_f32x4*>(yp);
      const qs_f32x4 mv = *reinterpret_cast<const qs_f32x4*>(mp);
#pragma unroll
      for (int e = 0; e < V; ++e) {
        d[e] = step_diff(yv[e], mv[e]);
        m[e] = mv[e];
      }
    } else {
      m[0] = mp[0];
      d[0] = step_diff(yp[0], m[0]);
    }
    int off = 0;
    if constexpr (MAP) off = offsets[(long long)img * hw + p];
    float* op = y_hat + base + i * V;
#pragma unroll
    for (int k = 0; k < kLadderMax; ++k) {
      if (k < nsteps) {
        float iv, sv;
        if constexpr (MAP) {
          const int idx = map_index(kb[k] + off) - kMapMin;
          sv = lut[idx];
          iv = lut[kMapLut + idx];
        } else {
          iv = inv[k];
          sv = st[k];
        }
        if constexpr (V == 4) {
          qs_f32x4 o;
#pragma unroll
          for (int e = 0; e < V; ++e) o[e] = step_value(step_round(d[e], iv), m[e], sv);
          *reinterpret_cast<qs_f32x4*>(op + k * plane) = o;
        } else {
          op[k * plane] = step_value(step_round(d[0], iv), m[0], sv);
        }
      }
    }
    next_unit(p, r, cu, dq, dr);
  }
}

static bool aligned(const void* p, uintptr_t a) { return reinterpret_cast<uintptr_t>(p) % a == 0; }

static bool step_sizes_ok(int n, int64_t hw, int c, int mu_stride) {
  return n >= 1 && n <= 65535 && hw >= 1 && c >= 1 && c % 4 == 0 && mu_stride >= c && mu_stride % 4 == 0;
}

static bool ladder_dequant_sizes_ok(int n, int64_t hw, int c, int mu_stride) {
  return n >= 1 && n <= 65535 && hw >= 1 && c >= 1 && (mu_stride == c || mu_stride == 2 * c);
}

// the three simple kernels: four vectors per thread
static unsigned step_blocks(int64_t nvec) { return (unsigned)std::min<int64_t>(std::max<int64_t>((nvec + 1023) / 1024, 1), 1024); }

// the ladder kernels: one unit per thread up to about `cap` workgroups in the launch, and the stride of next_unit
struct UnitGrid {
  dim3 grid;
  int dq, dr;
};

static UnitGrid unit_grid(int64_t hw, int cu, int threads, int cap, int n) {
  const long long nunit = (long long)hw * cu;
  const long long want = (nunit + threads - 1) / threads, most = std::max<long long>(1, cap / n);
  const dim3 grid((unsigned)std::min(want, most), (unsigned)n);
  const long long stride = (long long)grid.x * threads;
  return {grid, (int)(stride / cu), (int)(stride % cu)};
}

template <bool MAP, bool LDS, int V, bool REQ>
static int launch_ladder_cost_instance(int lds, hipStream_t s, const void* y, const float* mu, const unsigned short* tid0, int n,
                                       long long hw, int c, int mu_stride, const float* inv_step, const int* shift,
                                       const signed char* offsets, const float* lut, const int* kbase, int nsteps, const RansTables& T,
                                       const unsigned* cost_q, unsigned long long* cost) {
  if (LDS) SNTC_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(step_ladder_cost_kernel<MAP, LDS, V, REQ>), hipFuncAttributeMaxDynamicSharedMemorySize, lds));
  const UnitGrid g = unit_grid(hw, c / V, kLadderThreads, kLadderGrid, n);
  hipLaunchKernelGGL((step_ladder_cost_kernel<MAP, LDS, V, REQ>), g.grid, dim3(kLadderThreads), LDS ? lds : 0, s, y, mu, tid0, hw, c, mu_stride,
                     inv_step, shift, offsets, lut, kbase, nsteps, T, cost_q, g.dq, g.dr, cost);
  SNTC_HIP(hipGetLastError());
  return SNTC_OK;
}

// inv_step / shift (per image) or offsets / lut / kbase (MAP), the others null; REQ: y = the file's symbols, offsets = its map,
// kbase = the shifts; every check was made
template <bool MAP, bool REQ = false>
static int launch_ladder_cost(const void* y, const float* mu, int n, int64_t hw, int c, int mu_stride, const uint16_t* base_ids,
                              const float* inv_step, const int* shift, const signed char* offsets, const float* lut, const int* kbase,
                              int nsteps, const uint32_t* meta, int ntables, int total_entries, const uint32_t* cost_q, uint64_t* cost,
                              hipStream_t s) {
  if (int zrc = zero_async(cost, (size_t)n * nsteps * sizeof(uint64_t), s)) return zrc;
  const RansTables T{nullptr, reinterpret_cast<const uint2*>(meta), ntables, total_entries};   // the price replaces the cdf: never read
  const bool vec = aligned(y, 16) && aligned(mu, 16) && aligned(base_ids, 8);
  const long long tb = (long long)ntables * (long long)sizeof(uint2) + 4LL * total_entries;
  const bool lds = tb <= kLadderLdsLimit;
  const auto launch = lds ? (vec ? launch_ladder_cost_instance<MAP, true, 4, REQ> : launch_ladder_cost_instance<MAP, true, 1, REQ>)
                          : (vec ? launch_ladder_cost_instance<MAP, false, 4, REQ> : launch_ladder_cost_instance<MAP, false, 1, REQ>);
  return launch(lds ? (int)tb : 0, s, y, mu, base_ids, n, hw, c, mu_stride, inv_step, shift, offsets, lut, kbase, nsteps, T, cost_q,
                reinterpret_cast<unsigned long long*>(cost));
}

// inv_step / step (per image) or offsets / lut / kbase (MAP), the others null; every check was made
template <bool MAP>
static int launch_ladder_dequant(const float* y, const float* mu, int n, int64_t hw, int c, int mu_stride, const float* inv_step,
                                 const float* step, const signed char* offsets, const float* lut, const int* kbase, int nsteps,
                                 float* y_hat, hipStream_t s) {
  // 16-byte accesses: the three base pointers aligned and every row a multiple of 4 floats (c % 4 == 0; mu_stride is c or 2 c)
  const bool vec = c % 4 == 0 && aligned(y, 16) && aligned(mu, 16) && aligned(y_hat, 16);
  const UnitGrid g = unit_grid(hw, vec ? c / 4 : c, kDequantLadderThreads, kDequantLadderGrid, n);
  if (vec)
    hipLaunchKernelGGL((step_ladder_dequant_kernel<MAP, 4>), g.grid, dim3(kDequantLadderThreads), 0, s, y, mu, (long long)hw, c, mu_stride,
                       inv_step, step, offsets, lut, kbase, nsteps, g.dq, g.dr, y_hat);
  else
    hipLaunchKernelGGL((step_ladder_dequant_kernel<MAP, 1>), g.grid, dim3(kDequantLadderThreads), 0, s, y, mu, (long long)hw, c, mu_stride,
                       inv_step, step, offsets, lut, kbase, nsteps, g.dq, g.dr, y_hat);
  SNTC_HIP(hipGetLastError());
  return SNTC_OK;
}

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
  hipLaunchKernelGGL(step_symbols_kernel<false>, dim3(step_blocks(hw * (c / 4)), n), dim3(256), 0, (hipStream_t)stream, y, mu, base_ids,
                     (long long)hw, c, mu_stride, inv_step, shift, nullptr, nullptr, nullptr, symbols, table_ids);
  SNTC_HIP(hipGetLastError());
  return SNTC_OK;
}

extern "C" int sntc_step_map_symbols(const float* y, const float* mu, int n, int64_t hw, int c, int mu_stride, const uint16_t* base_ids,
                                     const int8_t* kmap, const float* lut, int32_t* symbols, uint16_t* table_ids, void* stream) {
  if (!y || !mu || !base_ids || !kmap || !lut || !symbols || !table_ids)
    return fail(SNTC_ERR_BAD_SHAPE, "sntc_step_map_symbols: null argument");
  if (!step_sizes_ok(n, hw, c, mu_stride))
    return fail(SNTC_ERR_BAD_SHAPE, "sntc_step_map_symbols: bad sizes (1 <= n <= 65535, c % 4 == 0, mu_stride >= c, mu_stride % 4 == 0)");
  if (!aligned(y, 16) || !aligned(mu, 16) || !aligned(symbols, 16) || !aligned(base_ids, 8) || !aligned(table_ids, 8) || !aligned(lut, 4))
    return fail(SNTC_ERR_BAD_SHAPE, "sntc_step_map_symbols: y / mu / symbols must be 16-byte aligned, the id arrays 8-byte aligned");
  hipLaunchKernelGGL(step_symbols_kernel<true>, dim3(step_blocks(hw * (c / 4)), n), dim3(256), 0, (hipStream_t)stream, y, mu, base_ids,
                     (long long)hw, c, mu_stride, nullptr, nullptr, nullptr, reinterpret_cast<const signed char*>(kmap), lut, symbols,
                     table_ids);
  SNTC_HIP(hipGetLastError());
  return SNTC_OK;
}

extern "C" int sntc_step_table_ids(const uint16_t* base_ids, int n, int64_t elems_per_image, const int32_t* shift, uint16_t* table_ids,
                                   void* stream) {
  if (!base_ids || !shift || !table_ids) return fail(SNTC_ERR_BAD_SHAPE, "sntc_step_table_ids: null argument");
  if (n < 1 || n > 65535 || elems_per_image < 1) return fail(SNTC_ERR_BAD_SHAPE, "sntc_step_table_ids: bad sizes (1 <= n <= 65535)");
  hipLaunchKernelGGL(step_table_ids_kernel<false>, dim3(step_blocks(elems_per_image / 4 + 1), n), dim3(256), 0, (hipStream_t)stream,
                     base_ids, (long long)elems_per_image, 1, shift, nullptr, table_ids);
  SNTC_HIP(hipGetLastError());
  return SNTC_OK;
}

extern "C" int sntc_step_map_table_ids(const uint16_t* base_ids, int n, int64_t hw, int c, const int8_t* kmap, uint16_t* table_ids,
                                       void* stream) {
  if (!base_ids || !kmap || !table_ids) return fail(SNTC_ERR_BAD_SHAPE, "sntc_step_map_table_ids: null argument");
  if (n < 1 || n > 65535 || hw < 1 || c < 1) return fail(SNTC_ERR_BAD_SHAPE, "sntc_step_map_table_ids: bad sizes (1 <= n <= 65535)");
  hipLaunchKernelGGL(step_table_ids_kernel<true>, dim3(step_blocks(hw * c / 4 + 1), n), dim3(256), 0, (hipStream_t)stream, base_ids,
                     (long long)hw, c, nullptr, reinterpret_cast<const signed char*>(kmap), table_ids);
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
  hipLaunchKernelGGL(dequant_step_kernel<false>, dim3(step_blocks(hw * (c / 4)), n), dim3(256), 0, (hipStream_t)stream, symbols, mu,
                     (long long)hw, c, mu_stride, step, nullptr, nullptr, y_hat);
  SNTC_HIP(hipGetLastError());
  return SNTC_OK;
}

extern "C" int sntc_dequant_step_map(const int32_t* symbols, const float* mu, int n, int64_t hw, int c, int mu_stride,
                                     const int8_t* kmap, const float* lut, float* y_hat, void* stream) {
  if (!symbols || !mu || !kmap || !lut || !y_hat) return fail(SNTC_ERR_BAD_SHAPE, "sntc_dequant_step_map: null argument");
  if (!step_sizes_ok(n, hw, c, mu_stride))
    return fail(SNTC_ERR_BAD_SHAPE, "sntc_dequant_step_map: bad sizes (1 <= n <= 65535, c % 4 == 0, mu_stride >= c, mu_stride % 4 == 0)");
  if (!aligned(symbols, 16) || !aligned(mu, 16) || !aligned(y_hat, 16) || !aligned(lut, 4))
    return fail(SNTC_ERR_BAD_SHAPE, "sntc_dequant_step_map: symbols / mu / y_hat must be 16-byte aligned");
  hipLaunchKernelGGL(dequant_step_kernel<true>, dim3(step_blocks(hw * (c / 4)), n), dim3(256), 0, (hipStream_t)stream, symbols, mu,
                     (long long)hw, c, mu_stride, nullptr, reinterpret_cast<const signed char*>(kmap), lut, y_hat);
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
  return launch_ladder_cost<false>(y, mu, n, hw, c, mu_stride, base_ids, inv_step, reinterpret_cast<const int*>(shift), nullptr, nullptr,
                                   nullptr, nsteps, meta, ntables, total_entries, cost_q, cost, (hipStream_t)stream);
}

extern "C" int sntc_step_map_ladder_cost(const float* y, const float* mu, int n, int64_t hw, int c, int mu_stride,
                                         const uint16_t* base_ids, const int8_t* offsets, const float* lut, const int32_t* base,
                                         int nsteps, const uint32_t* meta, int ntables, int total_entries, const uint32_t* cost_q,
                                         uint64_t* cost, void* stream) {
  if (!y || !mu || !base_ids || !offsets || !lut || !base || !meta || !cost_q || !cost)
    return fail(SNTC_ERR_BAD_SHAPE, "sntc_step_map_ladder_cost: null argument");
  if (!step_sizes_ok(n, hw, c, mu_stride))
    return fail(SNTC_ERR_BAD_SHAPE, "sntc_step_map_ladder_cost: bad sizes (1 <= n <= 65535, c % 4 == 0, mu_stride >= c, mu_stride % 4 == 0)");
  if (nsteps < 1 || nsteps > kLadderMax) return fail(SNTC_ERR_BAD_SHAPE, "sntc_step_map_ladder_cost: 1 <= nsteps <= 16");
  if (ntables <= kLadderTop || total_entries < 1)
    return fail(SNTC_ERR_BAD_SHAPE, "sntc_step_map_ladder_cost: the table set must hold the 64 tables of the scale ladder");
  if (!aligned(y, 4) || !aligned(mu, 4) || !aligned(base_ids, 2) || !aligned(lut, 4) || !aligned(base, 4) || !aligned(cost, 8))
    return fail(SNTC_ERR_BAD_SHAPE, "sntc_step_map_ladder_cost: misaligned argument");
  return launch_ladder_cost<true>(y, mu, n, hw, c, mu_stride, base_ids, nullptr, nullptr, reinterpret_cast<const signed char*>(offsets), lut,
                                  reinterpret_cast<const int*>(base), nsteps, meta, ntables, total_entries, cost_q, cost,
                                  (hipStream_t)stream);
}

extern "C" int sntc_step_requant_symbols(const int32_t* symbols, const float* mu, int n, int64_t hw, int c, int mu_stride,
                                         const uint16_t* base_ids, const int8_t* src_map, const int8_t* dst_map, const float* lut,
                                         int32_t* out_symbols, uint16_t* out_table_ids, void* stream) {
  if (!symbols || !mu || !base_ids || !src_map || !dst_map || !lut || !out_symbols || !out_table_ids)
    return fail(SNTC_ERR_BAD_SHAPE, "sntc_step_requant_symbols: null argument");
  if (!step_sizes_ok(n, hw, c, mu_stride))
    return fail(SNTC_ERR_BAD_SHAPE, "sntc_step_requant_symbols: bad sizes (1 <= n <= 65535, c % 4 == 0, mu_stride >= c, mu_stride % 4 == 0)");
  if (!aligned(symbols, 16) || !aligned(mu, 16) || !aligned(out_symbols, 16) || !aligned(base_ids, 8) || !aligned(out_table_ids, 8) ||
      !aligned(lut, 4))
    return fail(SNTC_ERR_BAD_SHAPE, "sntc_step_requant_symbols: symbols / mu / out_symbols must be 16-byte aligned, the id arrays 8-byte aligned");
  hipLaunchKernelGGL((step_symbols_kernel<true, true>), dim3(step_blocks(hw * (c / 4)), n), dim3(256), 0, (hipStream_t)stream, symbols, mu,
                     base_ids, (long long)hw, c, mu_stride, nullptr, nullptr, reinterpret_cast<const signed char*>(src_map),
                     reinterpret_cast<const signed char*>(dst_map), lut, out_symbols, out_table_ids);
  SNTC_HIP(hipGetLastError());
  return SNTC_OK;
}

extern "C" int sntc_step_requant_ladder_cost(const int32_t* symbols, const float* mu, int n, int64_t hw, int c, int mu_stride,
                                             const uint16_t* base_ids, const int8_t* src_map, const float* lut, const int32_t* shift,
                                             int nsteps, const uint32_t* meta, int ntables, int total_entries, const uint32_t* cost_q,
                                             uint64_t* cost, void* stream) {
  if (!symbols || !mu || !base_ids || !src_map || !lut || !shift || !meta || !cost_q || !cost)
    return fail(SNTC_ERR_BAD_SHAPE, "sntc_step_requant_ladder_cost: null argument");
  if (!step_sizes_ok(n, hw, c, mu_stride))
    return fail(SNTC_ERR_BAD_SHAPE, "sntc_step_requant_ladder_cost: bad sizes (1 <= n <= 65535, c % 4 == 0, mu_stride >= c, mu_stride % 4 == 0)");
  if (nsteps < 1 || nsteps > kLadderMax) return fail(SNTC_ERR_BAD_SHAPE, "sntc_step_requant_ladder_cost: 1 <= nsteps <= 16");
  if (ntables <= kLadderTop || total_entries < 1)
    return fail(SNTC_ERR_BAD_SHAPE, "sntc_step_requant_ladder_cost: the table set must hold the 64 tables of the scale ladder");
  if (!aligned(symbols, 4) || !aligned(mu, 4) || !aligned(base_ids, 2) || !aligned(lut, 4) || !aligned(shift, 4) || !aligned(cost, 8))
    return fail(SNTC_ERR_BAD_SHAPE, "sntc_step_requant_ladder_cost: misaligned argument");
  return launch_ladder_cost<true, true>(symbols, mu, n, hw, c, mu_stride, base_ids, nullptr, nullptr,
                                        reinterpret_cast<const signed char*>(src_map), lut, reinterpret_cast<const int*>(shift), nsteps, meta,
                                        ntables, total_entries, cost_q, cost, (hipStream_t)stream);
}

extern "C" int sntc_step_ladder_dequant(const float* y, const float* mu, int n, int64_t hw, int c, int mu_stride, const float* inv_step,
                                        const float* step, int nsteps, float* y_hat, void* stream) {
  if (!y || !mu || !inv_step || !step || !y_hat) return fail(SNTC_ERR_BAD_SHAPE, "sntc_step_ladder_dequant: null argument");
  if (nsteps < 1 || nsteps > kLadderMax) return fail(SNTC_ERR_BAD_SHAPE, "sntc_step_ladder_dequant: 1 <= nsteps <= 16");
  if (!ladder_dequant_sizes_ok(n, hw, c, mu_stride))
    return fail(SNTC_ERR_BAD_SHAPE, "sntc_step_ladder_dequant: bad sizes (1 <= n <= 65535, hw >= 1, c >= 1, mu_stride = c or 2 c)");
  if (!aligned(y, 4) || !aligned(mu, 4) || !aligned(inv_step, 4) || !aligned(step, 4) || !aligned(y_hat, 4))
    return fail(SNTC_ERR_BAD_SHAPE, "sntc_step_ladder_dequant: misaligned argument");
  return launch_ladder_dequant<false>(y, mu, n, hw, c, mu_stride, inv_step, step, nullptr, nullptr, nullptr, nsteps, y_hat,
                                      (hipStream_t)stream);
}

extern "C" int sntc_step_map_ladder_dequant(const float* y, const float* mu, int n, int64_t hw, int c, int mu_stride,
                                            const int8_t* offsets, const float* lut, const int32_t* base, int nsteps, float* y_hat,
                                            void* stream) {
  if (!y || !mu || !offsets || !lut || !base || !y_hat) return fail(SNTC_ERR_BAD_SHAPE, "sntc_step_map_ladder_dequant: null argument");
  if (nsteps < 1 || nsteps > kLadderMax) return fail(SNTC_ERR_BAD_SHAPE, "sntc_step_map_ladder_dequant: 1 <= nsteps <= 16");
  if (!ladder_dequant_sizes_ok(n, hw, c, mu_stride))
    return fail(SNTC_ERR_BAD_SHAPE, "sntc_step_map_ladder_dequant: bad sizes (1 <= n <= 65535, hw >= 1, c >= 1, mu_stride = c or 2 c)");
  if (!aligned(y, 4) || !aligned(mu, 4) || !aligned(lut, 4) || !aligned(base, 4) || !aligned(y_hat, 4))
    return fail(SNTC_ERR_BAD_SHAPE, "sntc_step_map_ladder_dequant: misaligned argument");
  return launch_ladder_dequant<true>(y, mu, n, hw, c, mu_stride, nullptr, nullptr, reinterpret_cast<const signed char*>(offsets), lut,
                                     reinterpret_cast<const int*>(base), nsteps, y_hat, (hipStream_t)stream);
}
