// msssim_grad.hip -- gradient of the (MS-)SSIM distortion D = 1 - mean_B q_i w.r.t. the reconstruction (DESIGN.md 4.6;
// the quality q_i is reference mshyper/models.py:321-331 -> tf.image.ssim / tf.image.ssim_multiscale, here on the
// UNROUNDED 0-255 floats a = (x + .5) 255, b = (x_hat cropped + .5) 255 that the SGA step's MSE path differentiates).
//
// Per image and channel: q = mean_c prod_k f_k^{w_k}, f_k = max(mean of the cs map of scale k (ssim map on the last scale), 0);
// single-scale SSIM (both sides < 160) is the plain mean of the ssim map.  A factor clamped at 0 has zero gradient and zeroes
// the gradient of its whole (image, channel) product; nothing divides by a zero factor.
//
//   sntc_msssim_inputs      x, x_hat -> a, b (cropped, unrounded) and the per-image SSE of sntc_distortion_grad
//   sntc_msssim_finish      the forward's [scales, 2, n, c] double sums -> q[n] and coef[scales, n, c] = d(weight q_i)/d(sum_k)
//   sntc_ssim_scale_grad    one scale, ONE launch: g(r) = coef ((w*A)(r) + a(r) (w*B)(r) + 2 b(r) (w*C)(r)) + pool adjoint
//   sntc_avgpool2_symmetric_grad   the pool adjoint on its own
//
// sntc_ssim_scale_grad is the fused variant: a workgroup owns a 16 x 16 tile of g, stages the 36 x 36 x C halo of a and b in
// LDS, and per channel forms the 26 x 26 tile of (A, B, C) = d map / d (mu_b, E[ab], E[a^2 + b^2]) with a separable row and
// column pass, then gathers it with the separable adjoint (full) correlation.  No coefficient map goes to HBM.
// The tile is centred first (one constant per tile and channel, subtracted from a and b): covariance and variances are
// shift-invariant, and E[x^2] - mu^2 of 0-255 data otherwise cancels in float32; the luminance term uses the true means.
#include <cmath>
#include "sntc_internal.h"

namespace sntc {

constexpr int kGWin = 11;
constexpr int kGTile = 16;
constexpr int kGOut = kGTile + kGWin - 1;    // 26: filter outputs that see the tile
constexpr int kGHalo = kGOut + kGWin - 1;    // 36: inputs those outputs see
constexpr int kMaxScales = 5;

struct GradWin {
  float w[kGWin];
};

struct FinishArgs {
  double count[kMaxScales];
  double weight[kMaxScales];
};

template <int C>
__global__ void __launch_bounds__(256) ssim_scale_grad_kernel(const float* __restrict__ a, const float* __restrict__ b, int h, int w,
                                                              GradWin win, float c1, float c2, const float* __restrict__ coef,
                                                              int use_lum, const float* __restrict__ g_coarse, int hs, int ws,
                                                              float out_scale, float* __restrict__ g) {
  __shared__ float sa[kGHalo * kGHalo * C];
  __shared__ float sb[kGHalo * kGHalo * C];
  __shared__ float4 srow[kGHalo * kGOut];              // row pass of the four moments; then the row pass of (A, B, C)
  __shared__ float scoef[3][kGOut * kGOut];
  const int img = blockIdx.z;
  const int ry0 = blockIdx.y * kGTile, rx0 = blockIdx.x * kGTile;
  const int ty = threadIdx.x >> 4, tx = threadIdx.x & 15;
  const int ry = ry0 + ty, rx = rx0 + tx;
  float* gout = g + (size_t)img * hs * ws * C;
  if (ry0 >= h || rx0 >= w) {                          // a tile of the padded margin (block-uniform)
    if (ry < hs && rx < ws) {
#pragma unroll
      for (int ch = 0; ch < C; ++ch) gout[((size_t)ry * ws + rx) * C + ch] = 0.0f;
    }
    return;
  }
  const int ho = h - kGWin + 1, wo = w - kGWin + 1;
  const float* ab = a + (size_t)img * h * w * C;
  const float* bb = b + (size_t)img * h * w * C;
  float shift[C];
  {
    const int cy = min(ry0 + kGTile / 2, h - 1), cx = min(rx0 + kGTile / 2, w - 1);
#pragma unroll
    for (int ch = 0; ch < C; ++ch) shift[ch] = ab[((size_t)cy * w + cx) * C + ch];
  }
  for (int p = threadIdx.x; p < kGHalo * kGHalo; p += 256) {
    const int ly = p / kGHalo, lx = p - ly * kGHalo;
    const int iy = ry0 - (kGWin - 1) + ly, ix = rx0 - (kGWin - 1) + lx;
    const bool inside = iy >= 0 && iy < h && ix >= 0 && ix < w;       // outside: feeds masked outputs only
#pragma unroll
    for (int ch = 0; ch < C; ++ch) {
      sa[p * C + ch] = inside ? ab[((size_t)iy * w + ix) * C + ch] - shift[ch] : 0.0f;
      sb[p * C + ch] = inside ? bb[((size_t)iy * w + ix) * C + ch] - shift[ch] : 0.0f;
    }
  }
  __syncthreads();
  float* srow2 = reinterpret_cast<float*>(srow);      // [3][kGOut][kGTile]
  constexpr int kRow2 = kGOut * kGTile;
  float gv[C];
#pragma unroll
  for (int ch = 0; ch < C; ++ch) {
    // moments, row pass: 36 rows x 26 output columns
    for (int it = threadIdx.x; it < kGHalo * kGOut; it += 256) {
      const int ly = it / kGOut, ox = it - ly * kGOut;
      float r0 = 0.f, r1 = 0.f, rxy = 0.f, rsq = 0.f;
#pragma unroll
      for (int j = 0; j < kGWin; ++j) {
        const int idx = (ly * kGHalo + ox + j) * C + ch;
        const float x = sa[idx], y = sb[idx], wj = win.w[j];
        r0 += wj * x;
        r1 += wj * y;
        rxy += wj * (x * y);
        rsq += wj * (x * x + y * y);
      }
      srow[it] = make_float4(r0, r1, rxy, rsq);
    }
    __syncthreads();
    // column pass and the partial derivatives of the map at each of the 26 x 26 filter outputs
    for (int it = threadIdx.x; it < kGOut * kGOut; it += 256) {
      const int py = it / kGOut, px = it - py * kGOut;
      float m0 = 0.f, m1 = 0.f, exy = 0.f, esq = 0.f;
#pragma unroll
      for (int i = 0; i < kGWin; ++i) {
        const float4 r = srow[(py + i) * kGOut + px];
        const float wi = win.w[i];
        m0 += wi * r.x;
        m1 += wi * r.y;
        exy += wi * r.z;
        esq += wi * r.w;
      }
      const int oy = ry0 - (kGWin - 1) + py, ox = rx0 - (kGWin - 1) + px;
      const bool valid = oy >= 0 && oy < ho && ox >= 0 && ox < wo;
      const float den = esq - (m0 * m0 + m1 * m1) + c2;             // var_a + var_b + c2 (centred moments)
      const float cs = (2.0f * exy - 2.0f * m0 * m1 + c2) / den;
      float lum = 1.0f, dlum = 0.0f;
      if (use_lum) {
        const float ta = m0 + shift[ch], tb = m1 + shift[ch];       // the true means
        const float den0 = ta * ta + tb * tb + c1;
        lum = (2.0f * ta * tb + c1) / den0;
        dlum = (2.0f * ta - lum * (2.0f * tb)) / den0;
      }
      const float inv = lum / den;
      scoef[0][it] = valid ? inv * (2.0f * m1 * cs - 2.0f * m0) + cs * dlum : 0.0f;   // d / d mu_b
      scoef[1][it] = valid ? 2.0f * inv : 0.0f;                                       // d / d E[ab]
      scoef[2][it] = valid ? -(inv * cs) : 0.0f;                                      // d / d E[a^2 + b^2]
    }
    __syncthreads();
    // adjoint correlation, row pass: input column r = rx0 + t collects outputs r - 10 .. r with weights w[10] .. w[0]
    for (int it = threadIdx.x; it < kRow2; it += 256) {
      const int py = it / kGTile, t = it - py * kGTile;
      float s0 = 0.f, s1 = 0.f, s2 = 0.f;
#pragma unroll
      for (int k = 0; k < kGWin; ++k) {
        const float wk = win.w[kGWin - 1 - k];
        const int idx = py * kGOut + t + k;
        s0 += wk * scoef[0][idx];
        s1 += wk * scoef[1][idx];
        s2 += wk * scoef[2][idx];
      }
      srow2[it] = s0;
      srow2[kRow2 + it] = s1;
      srow2[2 * kRow2 + it] = s2;
    }
    __syncthreads();
    {
      float s0 = 0.f, s1 = 0.f, s2 = 0.f;
#pragma unroll
      for (int k = 0; k < kGWin; ++k) {
        const float wk = win.w[kGWin - 1 - k];
        const int idx = (ty + k) * kGTile + tx;
        s0 += wk * srow2[idx];
        s1 += wk * srow2[kRow2 + idx];
        s2 += wk * srow2[2 * kRow2 + idx];
      }
      const int self = ((ty + kGWin - 1) * kGHalo + tx + kGWin - 1) * C + ch;
      gv[ch] = coef[(size_t)img * C + ch] * (s0 + sa[self] * s1 + 2.0f * sb[self] * s2);
    }
    __syncthreads();                                   // srow is rewritten by the next channel's row pass
  }
  if (ry >= hs || rx >= ws) return;
  const bool inside = ry < h && rx < w;
  const int hc = (h + 1) / 2, wc = (w + 1) / 2;
  // pool adjoint: a replicated last row / column of an odd size was read twice by the pool
  const float mult = 0.25f * (((h & 1) && ry == h - 1) ? 2.0f : 1.0f) * (((w & 1) && rx == w - 1) ? 2.0f : 1.0f);
#pragma unroll
  for (int ch = 0; ch < C; ++ch) {
    float v = 0.0f;
    if (inside) {
      v = gv[ch];
      if (g_coarse) v += mult * g_coarse[(((size_t)img * hc + (ry >> 1)) * wc + (rx >> 1)) * C + ch];
    }
    gout[((size_t)ry * ws + rx) * C + ch] = out_scale * v;
  }
}

// g_fine[n, h, w, c] = adjoint of the 2 x 2 symmetric-extended average pool applied to g_coarse[n, ceil(h/2), ceil(w/2), c]
__global__ void avgpool2_grad_kernel(const float* __restrict__ gc, int h, int w, int c, float* __restrict__ gf, int64_t total) {
  const int hc = (h + 1) / 2, wc = (w + 1) / 2;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int k = (int)(i % c);
    int64_t t = i / c;
    const int x = (int)(t % w);
    t /= w;
    const int y = (int)(t % h);
    const int64_t img = t / h;
    const float mult = 0.25f * (((h & 1) && y == h - 1) ? 2.0f : 1.0f) * (((w & 1) && x == w - 1) ? 2.0f : 1.0f);
    gf[i] = mult * gc[((img * hc + (y >> 1)) * wc + (x >> 1)) * c + k];
  }
}

// a = (x + .5) 255, b = (x_hat cropped + .5) 255, and sse[n] summed exactly as distortion_grad_kernel sums it (sga.hip)
__global__ void __launch_bounds__(256) msssim_inputs_kernel(const float* __restrict__ x, const float* __restrict__ xh, int h, int w,
                                                            int c, int hs, int ws, float* __restrict__ a, float* __restrict__ b,
                                                            double* __restrict__ sse) {
  const int img = blockIdx.y;
  const int64_t per_s = (int64_t)hs * ws * c;
  const int rowlen_s = ws * c;
  double acc = 0;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < per_s; i += (int64_t)gridDim.x * blockDim.x) {
    const int r = (int)(i / rowlen_s);
    const int o = (int)(i - (int64_t)r * rowlen_s);
    if (r < h && o < w * c) {
      const int64_t j = ((int64_t)img * h + r) * w * c + o;
      const float xv = x[j], hv = xh[img * per_s + i];
      const float d = hv - xv;
      const float d255 = 255.0f * d;
      acc += (double)(d255 * d255);
      a[j] = (xv + 0.5f) * 255.0f;
      b[j] = (hv + 0.5f) * 255.0f;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_down(acc, o, 64);
  __shared__ double part[4];
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) atomicAdd(sse + img, part[0] + part[1] + part[2] + part[3]);
}

__global__ void msssim_finish_kernel(const double* __restrict__ sums, FinishArgs fa, int scales, int n, int c, int single,
                                     double weight, double* __restrict__ q, float* __restrict__ coef) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double qi = 0.0;
  for (int ch = 0; ch < c; ++ch) {
    if (single) {                                       // tf.image.ssim: the plain mean of the ssim map, no clamp
      qi += sums[(size_t)i * c + ch] / fa.count[0];
      coef[(size_t)i * c + ch] = (float)(weight / c / fa.count[0]);
      continue;
    }
    double f[kMaxScales];
    double prod = 1.0;
    bool positive = true;
    for (int k = 0; k < scales; ++k) {
      const int which = k == scales - 1 ? 0 : 1;        // ssim on the last scale, cs on the others
      const double m = sums[(((size_t)k * 2 + which) * n + i) * c + ch] / fa.count[k];
      f[k] = m > 0.0 ? m : 0.0;
      positive = positive && f[k] > 0.0;
      prod *= pow(f[k], fa.weight[k]);
    }
    qi += prod;
    for (int k = 0; k < scales; ++k)                    // a clamped factor: zero gradient for the whole product, no 0 / 0
      coef[((size_t)k * n + i) * c + ch] = positive ? (float)(weight / c * prod * fa.weight[k] / f[k] / fa.count[k]) : 0.0f;
  }
  q[i] = qi / c;
}

}  // namespace sntc

using namespace sntc;

static int grad_blocks_for(int64_t total) {
  int64_t b = (total + 255) / 256;
  return (int)(b < 1 ? 1 : (b > 2048 ? 2048 : b));
}

extern "C" int sntc_msssim_inputs(const float* x, const float* x_hat, int n, int h, int w, int c, int hs, int ws, float* a,
                                  float* b, double* sse, void* stream) {
  if (!x || !x_hat || !a || !b || !sse) return fail(SNTC_ERR_BAD_SHAPE, "sntc_msssim_inputs: null argument");
  if (n < 1 || n > 65535 || h < 1 || w < 1 || c < 1 || hs < h || ws < w) return fail(SNTC_ERR_BAD_SHAPE, "sntc_msssim_inputs: bad sizes");
  hipStream_t s = (hipStream_t)stream;
  if (int zrc = zero_async(sse, sizeof(double) * n, s)) return zrc;
  int64_t blocks = ((int64_t)hs * ws * c + 255) / 256;                   // the grid of sntc_distortion_grad: the same partial sums
  if (blocks > 512) blocks = 512;
  hipLaunchKernelGGL(msssim_inputs_kernel, dim3((int)blocks, n), dim3(256), 0, s, x, x_hat, h, w, c, hs, ws, a, b, sse);
  SNTC_HIP(hipGetLastError());
  return SNTC_OK;
}

extern "C" int sntc_msssim_finish(const double* sums, const double* counts, const double* weights, int scales, int n, int c,
                                  double weight, double* q, float* coef, void* stream) {
  if (!sums || !counts || !q || !coef) return fail(SNTC_ERR_BAD_SHAPE, "sntc_msssim_finish: null argument");
  if (scales < 1 || scales > kMaxScales || n < 1 || c < 1) return fail(SNTC_ERR_BAD_SHAPE, "sntc_msssim_finish: bad sizes");
  if (scales > 1 && !weights) return fail(SNTC_ERR_BAD_SHAPE, "sntc_msssim_finish: multi-scale needs the scale weights");
  FinishArgs fa{};
  for (int k = 0; k < scales; ++k) {
    if (!(counts[k] >= 1.0)) return fail(SNTC_ERR_BAD_SHAPE, "sntc_msssim_finish: a scale without filter outputs");
    fa.count[k] = counts[k];
    fa.weight[k] = weights ? weights[k] : 1.0;
  }
  hipLaunchKernelGGL(msssim_finish_kernel, dim3((n + 63) / 64), dim3(64), 0, (hipStream_t)stream, sums, fa, scales, n, c,
                     scales == 1 ? 1 : 0, weight, q, coef);
  SNTC_HIP(hipGetLastError());
  return SNTC_OK;
}

extern "C" int sntc_ssim_scale_grad(const float* a, const float* b, int n, int h, int w, int c, float max_val, const float* coef,
                                    int use_lum, const float* g_coarse, int hs, int ws, float out_scale, float* g, void* stream) {
  if (!a || !b || !coef || !g) return fail(SNTC_ERR_BAD_SHAPE, "sntc_ssim_scale_grad: null argument");
  if (n < 1 || n > 65535 || h < kGWin || w < kGWin) return fail(SNTC_ERR_BAD_SHAPE, "sntc_ssim_scale_grad: image smaller than the 11 x 11 window");
  if (hs < h || ws < w) return fail(SNTC_ERR_BAD_SHAPE, "sntc_ssim_scale_grad: the gradient is smaller than the image");
  GradWin win;
  double s = 0, gw[kGWin];
  for (int i = 0; i < kGWin; ++i) {
    const double d = i - (kGWin - 1) / 2.0;
    gw[i] = std::exp(-0.5 * d * d / (1.5 * 1.5));
    s += gw[i];
  }
  for (int i = 0; i < kGWin; ++i) win.w[i] = (float)(gw[i] / s);
  const float c1 = (0.01f * max_val) * (0.01f * max_val), c2 = (0.03f * max_val) * (0.03f * max_val);
  const int gy = (hs + kGTile - 1) / kGTile;
  if (gy > 65535) return fail(SNTC_ERR_BAD_SHAPE, "sntc_ssim_scale_grad: image too tall");
  dim3 grid((ws + kGTile - 1) / kGTile, gy, n);
  hipStream_t st = (hipStream_t)stream;
  switch (c) {
    case 1:
      hipLaunchKernelGGL((ssim_scale_grad_kernel<1>), grid, dim3(256), 0, st, a, b, h, w, win, c1, c2, coef, use_lum, g_coarse, hs, ws,
                         out_scale, g);
      break;
    case 3:
      hipLaunchKernelGGL((ssim_scale_grad_kernel<3>), grid, dim3(256), 0, st, a, b, h, w, win, c1, c2, coef, use_lum, g_coarse, hs, ws,
                         out_scale, g);
      break;
    default: return fail(SNTC_ERR_UNSUPPORTED, "sntc_ssim_scale_grad: 1 or 3 channels");
  }
  SNTC_HIP(hipGetLastError());
  return SNTC_OK;
}

extern "C" int sntc_avgpool2_symmetric_grad(const float* g_coarse, int n, int h, int w, int c, float* g_fine, void* stream) {
  if (!g_coarse || !g_fine || n < 1 || h < 1 || w < 1 || c < 1) return fail(SNTC_ERR_BAD_SHAPE, "sntc_avgpool2_symmetric_grad: bad argument");
  const int64_t total = (int64_t)n * h * w * c;
  hipLaunchKernelGGL(avgpool2_grad_kernel, dim3(grad_blocks_for(total)), dim3(256), 0, (hipStream_t)stream, g_coarse, h, w, c, g_fine,
                     total);
  SNTC_HIP(hipGetLastError());
  return SNTC_OK;
}
