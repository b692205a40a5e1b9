// residual.hip -- the coded pixel residual layer (wire format 8, DESIGN.md 4.7 "residual layer"): a second layer over any
// hyperprior file that bounds the error of every decoded pixel by max_error = delta (0: lossless against the uint8 original).
// The reference never writes a file and has no per-pixel promise (mshyper/models.py:246-251: compression=False; its distortion is
// a mean, :313-317); this layer codes the integers q = sgn(r) ((|r| + delta) div (2 delta + 1)), r = x8 - base, with the 64 normal
// tables the model already holds, one table per (image, class), the class read off the base picture alone.  The rule is
// residual_rules.h, used by the three kernels here and by nothing else:
//   residual_quantize_kernel   x float, base uint8 -> q int32 and the histogram of q per (image, class), which the host prices
//                              under every table (entropy_coding.residual_choice) to choose by exact coded cost
//   residual_table_ids_kernel  base, the chosen table per (image, class) -> a table id per element; encoder and decoder share it
//   residual_apply_kernel      base, q -> x~ = clip(base + q (2 delta + 1), 0, 255), and a count of q no encoder writes
// All three are streams over an image taken as h rows of w c contiguous values.  Grid (workgroups per image, images): no workgroup
// straddles an image.  A thread's unit is V consecutive values of the image (V = 4: one 16-byte load of x or q, one 4-byte load of
// base; a unit may run over a row's end), V = 1 where a pointer or the image's size does not allow that: the same integers.
// The position (row, column, channel) of a unit's first value costs two 32-bit divisions; the values after it step.
// The class of a value needs four neighbours of the base picture (byte loads, clamped to the image; the lines are in the caches
// of the pass that reads the value itself).
//
// The histogram is workgroup-private in LDS, [8 c][511] counters (49 KB at c = 3: three workgroups per CU), zeroed at the start,
// fed by LDS atomics and flushed at the end with one integer global atomic per non-empty bin: every sum is an integer, so the
// result does not depend on the launch geometry or on the order the atomics arrive in.  On a smooth picture most values hit one
// bin of one class and its LDS atomics serialise; DESIGN.md 4.7 has the measurement.
#include <algorithm>
#include "sntc_internal.h"
#include "residual_rules.h"

namespace sntc {

constexpr int kResThreads = 256;
constexpr int kResGrid = 768;                               // workgroups of a launch, about: three per CU

// where a unit starts: its row, column and channel
struct ResPos {
  unsigned i, j, k;
};

__device__ __forceinline__ ResPos res_pos(unsigned e, unsigned wc, unsigned c) {
  ResPos p;
  p.i = e / wc;
  const unsigned r = e - p.i * wc;
  p.j = r / c;
  p.k = r - p.j * c;
  return p;
}

__device__ __forceinline__ void res_next(ResPos& p, unsigned w, unsigned c) {
  if (++p.k == c) {
    p.k = 0;
    if (++p.j == w) {
      p.j = 0;
      ++p.i;
    }
  }
}

// the activity level of value e of an image at position p: its four neighbours in the base picture, clamped to the image
__device__ __forceinline__ int res_level_at(const unsigned char* __restrict__ bi, unsigned e, const ResPos& p, unsigned h, unsigned w,
                                            unsigned c, unsigned wc) {
  const int left = bi[p.j > 0 ? e - c : e], right = bi[p.j + 1 < w ? e + c : e];
  const int up = bi[p.i > 0 ? e - wc : e], down = bi[p.i + 1 < h ? e + wc : e];
  return res_level(left, right, up, down);
}

template <int V>
__global__ void __launch_bounds__(kResThreads) residual_quantize_kernel(const float* __restrict__ x, const unsigned char* __restrict__ base,
                                                                        unsigned h, unsigned w, unsigned c, int delta, int* __restrict__ q,
                                                                        unsigned* __restrict__ hist) {
  extern __shared__ unsigned lh[];                           // [8 c][511]
  const unsigned nb = kResLevels * c * kResBins;
  for (unsigned i = threadIdx.x; i < nb; i += kResThreads) lh[i] = 0u;
  __syncthreads();
  const unsigned wc = w * c, E = h * wc, nunit = E / V;      // V == 4: E % 4 == 0 (host)
  const long long ib = (long long)blockIdx.y * E;
  const float* xi = x + ib;
  const unsigned char* bi = base + ib;
  int* qi = q + ib;
  const unsigned stride = gridDim.x * kResThreads;
  for (unsigned u = blockIdx.x * kResThreads + threadIdx.x; u < nunit; u += stride) {
    const unsigned e0 = u * V;
    float xv[V];
    unsigned char bv[V];
    int qv[V];
    if constexpr (V == 4) {
      const float4 t = *reinterpret_cast<const float4*>(xi + e0);
      const uchar4 b = *reinterpret_cast<const uchar4*>(bi + e0);
      xv[0] = t.x; xv[1] = t.y; xv[2] = t.z; xv[3] = t.w;
      bv[0] = b.x; bv[1] = b.y; bv[2] = b.z; bv[3] = b.w;
    } else {
      xv[0] = xi[e0];
      bv[0] = bi[e0];
    }
    ResPos p = res_pos(e0, wc, c);
#pragma unroll
    for (int v = 0; v < V; ++v) {
      qv[v] = res_quantize(res_pixel(xv[v]), (int)bv[v], delta);
      const int cls = res_class(res_level_at(bi, e0 + v, p, h, w, c, wc), (int)p.k, (int)c);
      atomicAdd(&lh[cls * kResBins + qv[v] + 255], 1u);
      res_next(p, w, c);
    }
    if constexpr (V == 4) {
      *reinterpret_cast<int4*>(qi + e0) = make_int4(qv[0], qv[1], qv[2], qv[3]);
    } else {
      qi[e0] = qv[0];
    }
  }
  __syncthreads();
  unsigned* out = hist + (size_t)blockIdx.y * nb;
  for (unsigned i = threadIdx.x; i < nb; i += kResThreads) {
    const unsigned cnt = lh[i];
    if (cnt) atomicAdd(&out[i], cnt);
  }
}

template <int V>
__global__ void __launch_bounds__(kResThreads) residual_table_ids_kernel(const unsigned char* __restrict__ base,
                                                                         const unsigned char* __restrict__ choice, unsigned h, unsigned w,
                                                                         unsigned c, unsigned short* __restrict__ ids) {
  __shared__ unsigned short tab[kResLevels * kResMaxChannels];
  const unsigned ncls = kResLevels * c;
  if (threadIdx.x < ncls)                                    // a byte beyond the ladder's last table can never index past it
    tab[threadIdx.x] = (unsigned short)min((int)choice[(size_t)blockIdx.y * ncls + threadIdx.x], kResTableTop);
  __syncthreads();
  const unsigned wc = w * c, E = h * wc, nunit = E / V;
  const long long ib = (long long)blockIdx.y * E;
  const unsigned char* bi = base + ib;
  unsigned short* oi = ids + ib;
  const unsigned stride = gridDim.x * kResThreads;
  for (unsigned u = blockIdx.x * kResThreads + threadIdx.x; u < nunit; u += stride) {
    const unsigned e0 = u * V;
    ResPos p = res_pos(e0, wc, c);
    unsigned short t[V];
#pragma unroll
    for (int v = 0; v < V; ++v) {
      t[v] = tab[res_class(res_level_at(bi, e0 + v, p, h, w, c, wc), (int)p.k, (int)c)];
      res_next(p, w, c);
    }
    if constexpr (V == 4) {
      *reinterpret_cast<ushort4*>(oi + e0) = make_ushort4(t[0], t[1], t[2], t[3]);
    } else {
      oi[e0] = t[0];
    }
  }
}

template <int V>
__global__ void __launch_bounds__(kResThreads) residual_apply_kernel(const unsigned char* __restrict__ base, const int* __restrict__ q,
                                                                     unsigned E, int delta, unsigned char* __restrict__ out,
                                                                     int* __restrict__ out_of_range) {
  const unsigned nunit = E / V;
  const long long ib = (long long)blockIdx.y * E;
  const unsigned char* bi = base + ib;
  const int* qi = q + ib;
  unsigned char* oi = out + ib;
  const int qmax = res_q_max(delta);
  const unsigned stride = gridDim.x * kResThreads;
  int bad = 0;
  for (unsigned u = blockIdx.x * kResThreads + threadIdx.x; u < nunit; u += stride) {
    const unsigned e0 = u * V;
    if constexpr (V == 4) {
      const int4 t = *reinterpret_cast<const int4*>(qi + e0);
      const uchar4 b = *reinterpret_cast<const uchar4*>(bi + e0);
      const int qv[4] = {t.x, t.y, t.z, t.w};
      const int bv[4] = {b.x, b.y, b.z, b.w};
      unsigned char o[4];
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        bad += (qv[v] > qmax || qv[v] < -qmax) ? 1 : 0;
        o[v] = (unsigned char)res_reconstruct(bv[v], qv[v], delta);
      }
      *reinterpret_cast<uchar4*>(oi + e0) = make_uchar4(o[0], o[1], o[2], o[3]);
    } else {
      const int t = qi[e0];
      bad += (t > qmax || t < -qmax) ? 1 : 0;
      oi[e0] = (unsigned char)res_reconstruct((int)bi[e0], t, delta);
    }
  }
  for (int off = 32; off > 0; off >>= 1) bad += __shfl_down(bad, off);
  if ((threadIdx.x & 63) == 0 && bad) atomicAdd(out_of_range, bad);
}

static inline bool res_aligned(const void* p, uintptr_t a) { return reinterpret_cast<uintptr_t>(p) % a == 0; }

// null: the sizes are good and *E holds an image's element count
static const char* res_sizes(int n, int h, int w, int c, int64_t* E) {
  if (n < 1 || n > 65535 || h < 1 || w < 1) return "bad sizes (1 <= n <= 65535, h >= 1, w >= 1)";
  if (c < 1 || c > kResMaxChannels) return "1 <= c <= 4";
  *E = (int64_t)h * w * c;
  if (*E > 0x7fffffffLL) return "an image holds at most 2^31 - 1 values";
  return nullptr;
}

// one unit per thread up to about kResGrid workgroups in the launch, grid-stride beyond
static dim3 res_grid(int64_t nunit, int n) {
  const int64_t want = (nunit + kResThreads - 1) / kResThreads, most = std::max<int64_t>(1, kResGrid / n);
  return dim3((unsigned)std::max<int64_t>(1, std::min(want, most)), (unsigned)n);
}

}  // namespace sntc

using namespace sntc;

extern "C" int sntc_residual_quantize(const float* x, const uint8_t* base, int n, int h, int w, int c, int max_error, int32_t* q,
                                      uint32_t* hist, void* stream) {
  if (!x || !base || !q || !hist) return fail(SNTC_ERR_BAD_SHAPE, "sntc_residual_quantize: null argument");
  int64_t E = 0;
  if (const char* why = res_sizes(n, h, w, c, &E)) return fail(SNTC_ERR_BAD_SHAPE, std::string("sntc_residual_quantize: ") + why);
  if (max_error < 0 || max_error > kResMaxError) return fail(SNTC_ERR_BAD_SHAPE, "sntc_residual_quantize: 0 <= max_error <= 127");
  if (!res_aligned(x, 4) || !res_aligned(q, 4) || !res_aligned(hist, 4))
    return fail(SNTC_ERR_BAD_SHAPE, "sntc_residual_quantize: misaligned argument");
  hipStream_t s = (hipStream_t)stream;
  const size_t lds = (size_t)kResLevels * c * kResBins * sizeof(unsigned);
  if (int zrc = zero_async(hist, (size_t)n * lds, s)) return zrc;
  const bool vec = E % 4 == 0 && res_aligned(x, 16) && res_aligned(q, 16) && res_aligned(base, 4);
  const auto kernel = vec ? residual_quantize_kernel<4> : residual_quantize_kernel<1>;
  SNTC_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(kernel, res_grid(vec ? E / 4 : E, n), dim3(kResThreads), lds, s, x, base, (unsigned)h, (unsigned)w, (unsigned)c,
                     max_error, q, hist);
  SNTC_HIP(hipGetLastError());
  return SNTC_OK;
}

extern "C" int sntc_residual_table_ids(const uint8_t* base, const uint8_t* choice, int n, int h, int w, int c, uint16_t* table_ids,
                                       void* stream) {
  if (!base || !choice || !table_ids) return fail(SNTC_ERR_BAD_SHAPE, "sntc_residual_table_ids: null argument");
  int64_t E = 0;
  if (const char* why = res_sizes(n, h, w, c, &E)) return fail(SNTC_ERR_BAD_SHAPE, std::string("sntc_residual_table_ids: ") + why);
  if (!res_aligned(table_ids, 2)) return fail(SNTC_ERR_BAD_SHAPE, "sntc_residual_table_ids: misaligned argument");
  const bool vec = E % 4 == 0 && res_aligned(base, 4) && res_aligned(table_ids, 8);
  const auto kernel = vec ? residual_table_ids_kernel<4> : residual_table_ids_kernel<1>;
  hipLaunchKernelGGL(kernel, res_grid(vec ? E / 4 : E, n), dim3(kResThreads), 0, (hipStream_t)stream, base, choice, (unsigned)h,
                     (unsigned)w, (unsigned)c, table_ids);
  SNTC_HIP(hipGetLastError());
  return SNTC_OK;
}

extern "C" int sntc_residual_apply(const uint8_t* base, const int32_t* q, int n, int h, int w, int c, int max_error, uint8_t* out,
                                   int32_t* out_of_range, void* stream) {
  if (!base || !q || !out || !out_of_range) return fail(SNTC_ERR_BAD_SHAPE, "sntc_residual_apply: null argument");
  int64_t E = 0;
  if (const char* why = res_sizes(n, h, w, c, &E)) return fail(SNTC_ERR_BAD_SHAPE, std::string("sntc_residual_apply: ") + why);
  if (max_error < 0 || max_error > kResMaxError) return fail(SNTC_ERR_BAD_SHAPE, "sntc_residual_apply: 0 <= max_error <= 127");
  if (!res_aligned(q, 4) || !res_aligned(out_of_range, 4)) return fail(SNTC_ERR_BAD_SHAPE, "sntc_residual_apply: misaligned argument");
  hipStream_t s = (hipStream_t)stream;
  if (int zrc = zero_async(out_of_range, sizeof(int32_t), s)) return zrc;
  const bool vec = E % 4 == 0 && res_aligned(base, 4) && res_aligned(q, 16) && res_aligned(out, 4);
  const auto kernel = vec ? residual_apply_kernel<4> : residual_apply_kernel<1>;
  hipLaunchKernelGGL(kernel, res_grid(vec ? E / 4 : E, n), dim3(kResThreads), 0, s, base, q, (unsigned)E, max_error, out, out_of_range);
  SNTC_HIP(hipGetLastError());
  return SNTC_OK;
}
