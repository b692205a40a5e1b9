// quant_step_ladder.hip -- the DEQUANTISED latents of every candidate of a step ladder in one pass ("quality
// target").  The reference quantises y - mu with step 1 and decodes y_hat = round(y - mu) + mu (mshyper/models.py:273-279, one
// decode per evaluation); quant_step.hip generalises that line to a step off the scale ladder, and its ladder-cost kernel prices
// up to 16 candidate steps from one read of y / mu / ids.  These kernels are the distortion side of the same ladder: what each
// candidate DECODES to.  Per element and candidate j, with the rules of step_rules.h and nothing else,
//   s     = step_round(step_diff(y, mu), inv_step[j])        never clamped: the symbol coded_cost decodes, not the file's
//   y_hat = step_value(s, mu, step[j])                       16-bit escape
// written to y_hat[j][image][position][channel]: candidate j is a contiguous batch of n latents the decoder takes as it is, so
// the nsteps candidates of n images are ONE decoder batch of nsteps n.  Candidate plane j equals sntc_dequant_step of
// sntc_step_symbols at that step (sntc_dequant_step_map of sntc_step_map_symbols for the map kernel), bit for bit.
//
// Shape: a store stream.  y and mu are read once per launch (8 bytes per element), every load feeds nsteps stores (4 nsteps
// bytes per element): with 16 candidates 64 bytes out per 8 in, the roof is HBM write bandwidth.  A thread's unit is V elements
// of one position: V = 4 is one 16-byte load of y and of mu and nsteps 16-byte stores; V = 1 where a pointer is not 16-byte
// aligned or c % 4 != 0.  No atomics, no LDS; the map kernel reads the 65-entry step table through the vector cache.
#include <algorithm>
#include "sntc_internal.h"
#include "step_rules.h"

namespace sntc {

constexpr int kDequantLadderMax = 16;                       // candidates of one launch (their steps live in scalar registers)
constexpr int kDequantLadderThreads = 256;
constexpr int kDequantLadderGrid = 2048;                    // workgroups of a launch, about: 8 per CU, grid-stride beyond

typedef float ql_f32x4 __attribute__((ext_vector_type(4)));

// grid (workgroups per image, n): no workgroup straddles an image.  (position, unit in the position) advance by the launch's
// stride as (dq, dr): no division in the loop.  MAP: candidate j's index at position p is map_index(kbase[j] + offsets[p]), its
// step and inverse step lut[0][.] and lut[1][.]; else a[j] = inv_step[j], b[j] = step[j], uniform.
template <bool MAP, int V>
__global__ void __launch_bounds__(kDequantLadderThreads) step_ladder_dequant_kernel(
    const float* __restrict__ y, const float* __restrict__ mu, long long hw, int c, int mu_stride, const float* __restrict__ a,
    const float* __restrict__ b, const signed char* __restrict__ offsets, const int* __restrict__ kbase, int nsteps, int dq, int dr,
    float* __restrict__ y_hat) {
  float inv[kDequantLadderMax], st[kDequantLadderMax];
  int kb[kDequantLadderMax];
#pragma unroll
  for (int k = 0; k < kDequantLadderMax; ++k) {
    if (MAP) {
      kb[k] = k < nsteps ? min(max(kbase[k], -256), 256) : 0;  // beyond +-160 every int8 offset clips to the same end: same result,
                                                               // and base + offset cannot overflow
    } else {
      inv[k] = k < nsteps ? a[k] : 0.0f;
      st[k] = k < nsteps ? b[k] : 0.0f;
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
    if (V == 4) {
      const ql_f32x4 yv = *reinterpret_cast<const ql_f32x4*>(yp);
      const ql_f32x4 mv = *reinterpret_cast<const ql_f32x4*>(mp);
#pragma unroll
      for (int e = 0; e < V; ++e) {
        d[e] = step_diff(yv[e], mv[e]);
        m[e] = mv[e];
      }
    } else {
      m[0] = mp[0];
      d[0] = step_diff(yp[0], m[0]);
    }
    const int off = MAP ? offsets[(long long)img * hw + p] : 0;
    float* op = y_hat + base + i * V;
#pragma unroll
    for (int k = 0; k < kDequantLadderMax; ++k) {
      if (k < nsteps) {
        float iv, sv;
        if (MAP) {
          const int idx = map_index(kb[k] + off) - kMapMin;
          sv = a[idx];
          iv = a[kMapLut + idx];
        } else {
          iv = inv[k];
          sv = st[k];
        }
        if (V == 4) {
          ql_f32x4 o;
#pragma unroll
          for (int e = 0; e < V; ++e) o[e] = step_value(step_round(d[e], iv), m[e], sv);
          *reinterpret_cast<ql_f32x4*>(op + k * plane) = o;
        } else {
          op[k * plane] = step_value(step_round(d[0], iv), m[0], sv);
        }
      }
    }
    p += dq;
    r += dr;
    if (r >= cu) {
      r -= cu;
      ++p;
    }
  }
}

static bool ql_aligned(const void* p, uintptr_t a) { return reinterpret_cast<uintptr_t>(p) % a == 0; }

// a = inv_step, b = step (offsets == nullptr) or a = lut, b unused, with offsets / kbase (the map); every check was made
template <bool MAP>
static int launch_ladder_dequant(const float* y, const float* mu, int n, int64_t hw, int c, int mu_stride, const float* a, const float* b,
                                 const signed char* offsets, const int* kbase, int nsteps, float* y_hat, hipStream_t s) {
  // 16-byte accesses: the three base pointers aligned and every row a multiple of 4 floats (c % 4 == 0; mu_stride is c or 2 c)
  const bool vec = c % 4 == 0 && ql_aligned(y, 16) && ql_aligned(mu, 16) && ql_aligned(y_hat, 16);
  const int cu = vec ? c / 4 : c;
  const long long nunit = (long long)hw * cu;
  const long long want = (nunit + kDequantLadderThreads - 1) / kDequantLadderThreads, most = std::max<long long>(1, kDequantLadderGrid / n);
  const dim3 grid((unsigned)std::min(want, most), (unsigned)n);
  const long long stride = (long long)grid.x * kDequantLadderThreads;
  const int dq = (int)(stride / cu), dr = (int)(stride % cu);
  if (vec)
    hipLaunchKernelGGL((step_ladder_dequant_kernel<MAP, 4>), grid, dim3(kDequantLadderThreads), 0, s, y, mu, (long long)hw, c, mu_stride, a,
                       b, offsets, kbase, nsteps, dq, dr, y_hat);
  else
    hipLaunchKernelGGL((step_ladder_dequant_kernel<MAP, 1>), grid, dim3(kDequantLadderThreads), 0, s, y, mu, (long long)hw, c, mu_stride, a,
                       b, offsets, kbase, nsteps, dq, dr, y_hat);
  SNTC_HIP(hipGetLastError());
  return SNTC_OK;
}

static bool ladder_dequant_sizes_ok(int n, int64_t hw, int c, int mu_stride) {
  return n >= 1 && n <= 65535 && hw >= 1 && c >= 1 && (mu_stride == c || mu_stride == 2 * c);
}

}  // namespace sntc

using namespace sntc;

extern "C" int sntc_step_ladder_dequant(const float* y, const float* mu, int n, int64_t hw, int c, int mu_stride, const float* inv_step,
                                        const float* step, int nsteps, float* y_hat, void* stream) {
  if (!y || !mu || !inv_step || !step || !y_hat) return fail(SNTC_ERR_BAD_SHAPE, "sntc_step_ladder_dequant: null argument");
  if (nsteps < 1 || nsteps > kDequantLadderMax) return fail(SNTC_ERR_BAD_SHAPE, "sntc_step_ladder_dequant: 1 <= nsteps <= 16");
  if (!ladder_dequant_sizes_ok(n, hw, c, mu_stride))
    return fail(SNTC_ERR_BAD_SHAPE, "sntc_step_ladder_dequant: bad sizes (1 <= n <= 65535, hw >= 1, c >= 1, mu_stride = c or 2 c)");
  if (!ql_aligned(y, 4) || !ql_aligned(mu, 4) || !ql_aligned(inv_step, 4) || !ql_aligned(step, 4) || !ql_aligned(y_hat, 4))
    return fail(SNTC_ERR_BAD_SHAPE, "sntc_step_ladder_dequant: misaligned argument");
  return launch_ladder_dequant<false>(y, mu, n, hw, c, mu_stride, inv_step, step, nullptr, nullptr, nsteps, y_hat, (hipStream_t)stream);
}

extern "C" int sntc_step_map_ladder_dequant(const float* y, const float* mu, int n, int64_t hw, int c, int mu_stride,
                                            const int8_t* offsets, const float* lut, const int32_t* base, int nsteps, float* y_hat,
                                            void* stream) {
  if (!y || !mu || !offsets || !lut || !base || !y_hat) return fail(SNTC_ERR_BAD_SHAPE, "sntc_step_map_ladder_dequant: null argument");
  if (nsteps < 1 || nsteps > kDequantLadderMax) return fail(SNTC_ERR_BAD_SHAPE, "sntc_step_map_ladder_dequant: 1 <= nsteps <= 16");
  if (!ladder_dequant_sizes_ok(n, hw, c, mu_stride))
    return fail(SNTC_ERR_BAD_SHAPE, "sntc_step_map_ladder_dequant: bad sizes (1 <= n <= 65535, hw >= 1, c >= 1, mu_stride = c or 2 c)");
  if (!ql_aligned(y, 4) || !ql_aligned(mu, 4) || !ql_aligned(lut, 4) || !ql_aligned(base, 4) || !ql_aligned(y_hat, 4))
    return fail(SNTC_ERR_BAD_SHAPE, "sntc_step_map_ladder_dequant: misaligned argument");
  return launch_ladder_dequant<true>(y, mu, n, hw, c, mu_stride, lut, nullptr, reinterpret_cast<const signed char*>(offsets),
                                     reinterpret_cast<const int*>(base), nsteps, y_hat, (hipStream_t)stream);
}
