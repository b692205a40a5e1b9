// residual_rules.h -- the rule of the coded pixel residual layer (wire format 8, DESIGN.md 4.7 "residual layer"), one function per
// step, shared by the three kernels of residual.hip; tests/residual_cases.py restates it in numpy.  Integer arithmetic from the
// pixel on.  x8 = the original quantised to uint8 as sntc_pixels_sse quantises it, b = the decoded base pixel, delta = max_error
// in 0 .. 127, m = 2 delta + 1:
//   quantiser       r = x8 - b,  q = sgn(r) ((|r| + delta) div m)                     res_quantize
//   reconstruction  x~ = clip(b + q m, 0, 255)                                        res_reconstruct;  |x8 - x~| <= delta
//   class           a = |b(i, j+1, k) - b(i, j-1, k)| + |b(i+1, j, k) - b(i-1, j, k)|, neighbours clamped to the image,
//                   level = 0 if a == 0 else min(7, floor(log2 a) + 1),  class = level C + k      res_level / res_class
// The class reads the base picture alone, so the decoder forms it before it has a residual.
#pragma once
#include <hip/hip_runtime.h>

namespace sntc {

constexpr int kResLevels = 8;                               // activity levels of the class rule
constexpr int kResBins = 511;                               // q + 255 for q in [-255, 255]
constexpr int kResMaxError = 127;
constexpr int kResMaxChannels = 4;
constexpr int kResTableTop = 63;                            // last of the 64 normal tables a choice byte may name

// the uint8 pixel of a float image value: (v + .5) 255, round half to even, saturate (to_pixel of pixel.hip)
__host__ __device__ __forceinline__ int res_pixel(float v) {
  const float p = rintf((v + 0.5f) * 255.0f);
  return (int)fminf(fmaxf(p, 0.0f), 255.0f);
}

__host__ __device__ __forceinline__ int res_quantize(int x8, int b, int delta) {
  const int r = x8 - b, a = r < 0 ? -r : r;
  const int q = (a + delta) / (2 * delta + 1);
  return r < 0 ? -q : q;
}

// the largest |q| res_quantize can produce at this delta; a decoded q beyond it is corrupt (and clips anyway)
__host__ __device__ __forceinline__ int res_q_max(int delta) { return (255 + delta) / (2 * delta + 1); }

// any int32 q: beyond +-256 the sum leaves [0, 255] whatever b and m >= 1 are, so q is clamped there first and the
// product cannot overflow
__host__ __device__ __forceinline__ int res_reconstruct(int b, int q, int delta) {
  const int qc = q < -256 ? -256 : (q > 256 ? 256 : q);
  const int v = b + qc * (2 * delta + 1);
  return v < 0 ? 0 : (v > 255 ? 255 : v);
}

__host__ __device__ __forceinline__ int res_level(int left, int right, int up, int down) {
  const int dx = right - left, dy = down - up;
  const int a = (dx < 0 ? -dx : dx) + (dy < 0 ? -dy : dy);           // 0 .. 510
  int level = 0;
  for (int t = a; t > 0; t >>= 1) ++level;                           // floor(log2 a) + 1, at most 9
  return level < kResLevels - 1 ? level : kResLevels - 1;
}

__host__ __device__ __forceinline__ int res_class(int level, int k, int c) { return level * c + k; }

}  // namespace sntc
