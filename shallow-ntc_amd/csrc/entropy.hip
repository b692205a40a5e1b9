// entropy.hip -- rate estimates of the two entropy models (compression=False paths).
//
// Both kernels are pure HBM streams: read each latent once, write the rounded value once, and
// reduce -log2 p per image.  One thread handles 4 consecutive channels (16-B loads); per-thread
// partial sums are kept in double, reduced across the wave with shuffles, across the block through
// LDS, then one double atomic per block and image (DESIGN.md "entropy scans").
//
// Numerics follow tfc's UniformNoiseAdapter:
//   log p(v) = big + log1p(-exp(small - big)),  (big, small) = (log cdf(v+.5), log cdf(v-.5)) left of
//   the median and (log sf(v-.5), log sf(v+.5)) right of it.  For the zero-mean normal and for the
//   logistic-sigmoid cumulative "right of the median" is simply upper > 0, and sf(x) = cdf(-x).
#include <algorithm>
#include <cmath>
#include <vector>
#include "device_math.h"

namespace sntc {

typedef int i32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float log_diff_exp(float big, float small) {
  return big + log1pf(-expf(small - big));
}

// -log2 P(v) for N(0, sigma) convolved with U(-.5, .5) -- the reference formulation (tfc's adapter over TFP's log_ndtr, SURVEY.md
// A.6), kept for the SGA / training kernels' callers and as the A/B of the rewritten scan below
__device__ __forceinline__ float normal_bits(float v, float sigma) {
  const float hi = (v + 0.5f) / sigma;
  const float lo = (v - 0.5f) / sigma;
  const bool right = hi > 0.0f;
  const float a = right ? -lo : hi;
  const float b = right ? -hi : lo;
  return -log_diff_exp(log_ndtr_f(a), log_ndtr_f(b)) * kInvLn2;
}

// ---- round 6: the same quantity in ~1/4 of the instructions (528 vector instructions per element) ----
// P(v) = Phi((a + .5) / s) - Phi((a - .5) / s) with a = |v| (the density is even: "right of the median take the survival pair" of
// A.6 IS this symmetry).  With z_l = (a - .5) / s, z_u = (a + .5) / s, erfc(x) = exp(-x^2) erfcx(x) and z_u^2 - z_l^2 = 2 a / s^2:
//   a >= 1:  ln P = -z_l^2 / 2 + ln( [erfcx(z_l / sqrt 2) - exp(-a / s^2) erfcx(z_u / sqrt 2)] / 2 )      (no underflow in any tail)
//   a == 0:  ln P = ln(1 - exp(-z_u^2 / 2) erfcx(z_u / sqrt 2))                                            (= ln erf(z_u / sqrt 2))
// i.e. ONE exp, two erfcx (a 12th-degree polynomial in q = (x - 2) / (x + 2) over 1 + 2x: two v_rcp_f32 and 13 fma each) and one log
// per symbol, the same instruction stream on every lane (selects, no divergent branches); the far tails need no separate series --
// erfcx is smooth to infinity.  Against float64 (2e6 synthetic latents, emulated in numpy before it was written): sum of bits
// within 2e-8 relative, the same as the formulation above (whose bias was the rounding of 1 / ln 2: carried here in two terms).
// That is a figure of the SUM.  One symbol (the same emulation on the plane of tests/test_hip_rate_plane.py: 102 scales x the
// integers -70 .. 70 and out to +-5000): min(abs, rel) error up to 1.0e-5 -- at sigma = 256, where cl and e agree to three digits
// (v = -10: 9.32694 for 9.32684 bits) -- against 6.0e-6 for the reference formulation at float32; the test holds both to 2.4e-5.
__device__ __forceinline__ float exp_f(float x) {          // exp(x), ~1.5 ulp; underflows to 0, overflows to inf
  const float hi = x * 1.44269502162933349609375f;
  const float lo = fmaf(x, 1.44269502162933349609375f, -hi) + x * 1.925963033500011e-8f;   // log2 e = hi part + 1.926e-8
  return __builtin_amdgcn_exp2f(hi) * fmaf(lo, 0.693147182464599609375f, 1.0f);
}

__device__ __forceinline__ float erfcx_pos(float x) {      // exp(x^2) erfc(x) for x >= 0, <= 2.5e-7 relative (fit: tools/fit_erfcx.py)
  const float q = (x - 2.0f) * __builtin_amdgcn_rcpf(x + 2.0f);
  float p = -2.0108929675188847e-05f;
  p = fmaf(p, q, 6.310018216026947e-05f);
  p = fmaf(p, q, 0.00022110545251052827f);
  p = fmaf(p, q, -0.0003571778943296522f);
  p = fmaf(p, q, -0.0014635116094723344f);
  p = fmaf(p, q, 0.0012166654923930764f);
  p = fmaf(p, q, 0.008724294602870941f);
  p = fmaf(p, q, -0.008018636144697666f);
  p = fmaf(p, q, -0.054220184683799744f);
  p = fmaf(p, q, 0.1640494018793106f);
  p = fmaf(p, q, -0.1660303920507431f);
  p = fmaf(p, q, -0.0927637591958046f);
  p = fmaf(p, q, 1.2769783735275269f);
  return p * __builtin_amdgcn_rcpf(fmaf(2.0f, x, 1.0f));
}

// -log2 P for |v| = a under N(0, 1 / inv_sigma) convolved with U(-.5, .5)
__device__ __forceinline__ float normal_bits_fast(float a, float inv_sigma) {
  const float zl = (a - 0.5f) * inv_sigma, zu = (a + 0.5f) * inv_sigma;
  const float cu = erfcx_pos(zu * 0.70710678118654752f);
  const float cl = erfcx_pos(fabsf(zl) * 0.70710678118654752f);
  const bool nz = a >= 1.0f;
  const float t = exp_f(-(nz ? a * inv_sigma * inv_sigma : 0.5f * zu * zu));
  const float e = t * cu;
  // a == 0 and e small: ln(1 - e) by its series (1 - e would round away what is being measured)
  const float ser = -e * fmaf(e, fmaf(e, fmaf(e, fmaf(e, 0.2f, 0.25f), 0.33333334f), 0.5f), 1.0f);
  const float d = nz ? 0.5f * (cl - e) : 1.0f - e;
  float lnp = logf(d);
  lnp = (!nz && e < 0.0625f) ? ser : lnp;
  lnp = nz ? fmaf(-0.5f * zl, zl, lnp) : lnp;
  return -fmaf(lnp, 1.925963033500011e-8f, lnp * 1.44269502162933349609375f);
}

// grid (blocks_per_image, n).  4 channels per thread and step; c % 4 == 0.  (p, ch) of a thread's vectors advance incrementally
// by the launch's stride (dq pixels + dr channel quads per step: no division in the loop).
// VALUES: explicit-sample mode (y holds the samples, possibly non-integer: the reference formulation; nothing is written back).
template <bool VALUES>
__global__ void __launch_bounds__(256) scale_normal_kernel(const float* __restrict__ y, const float* __restrict__ hyper,
                                                           int64_t hw, int c, float* __restrict__ y_hat,
                                                           int32_t* __restrict__ symbols, double* __restrict__ bits,
                                                           int dq, int dr) {
  constexpr bool values_only = VALUES;
  const int img = blockIdx.y;
  const int64_t per = hw * c;
  const int c4 = c >> 2;
  const int64_t nvec = hw * c4;
  const float* yb = y + img * per;
  const float* hb = hyper + img * per * 2;
  float* ob = y_hat ? y_hat + img * per : nullptr;
  int32_t* sb = symbols ? symbols + img * per : nullptr;
  double acc = 0.0;
  const int64_t i0 = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  int64_t p = i0 / c4;
  int q4 = (int)(i0 - p * c4);
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = i0; i < nvec; i += stride) {
    const int ch = q4 << 2;
    const f32x4 yv = *reinterpret_cast<const f32x4*>(yb + p * c + ch);
    const f32x4 mu = *reinterpret_cast<const f32x4*>(hb + p * 2 * c + ch);
    const f32x4 raw = *reinterpret_cast<const f32x4*>(hb + p * 2 * c + c + ch);
    f32x4 out;
    i32x4 sym;
    float b = 0.0f;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      // indexes = exp(raw) (mshyper/models.py:274-276), clamp to [0, 63], sigma = SCALE_FN(idx); 1 / sigma directly
      const float idx = fminf(exp_f(raw[e]), 63.0f);
      const float inv_sigma = exp_f(-fmaf(kScaleFactor, idx, kLogScaleMin));
      const float d = yv[e] - mu[e];
      const float v = values_only ? d : rintf(d);
      out[e] = v + mu[e];
      sym[e] = (int)v;
      b += values_only ? normal_bits(v, 1.0f / inv_sigma) : normal_bits_fast(fabsf(v), inv_sigma);
    }
    acc += (double)b;
    if (!values_only) {
      *reinterpret_cast<f32x4*>(ob + p * c + ch) = out;
      if (sb) *reinterpret_cast<i32x4*>(sb + p * c + ch) = sym;
    }
    p += dq;
    q4 += dr;
    if (q4 >= c4) { q4 -= c4; ++p; }
  }
  block_sum_to(acc, bits + img);
}

// `hstride`: floats per pixel of `hyper` -- 2 c for the hyper-synthesis' [mu | raw sigma] rows, c for a compact mu (the mean-only
// hyper-synthesis of the decoder, sntc_dequant_mean)
__global__ void __launch_bounds__(256) dequant_kernel(const int32_t* __restrict__ symbols, const float* __restrict__ hyper,
                                                      int64_t npix, int c, int hstride, float* __restrict__ y_hat) {
  const int c4 = c >> 2;
  const int64_t nvec = npix * c4;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < nvec; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t p = i / c4;
    const int ch = (int)(i - p * c4) << 2;
    const i32x4 s = *reinterpret_cast<const i32x4*>(symbols + p * c + ch);
    const f32x4 mu = *reinterpret_cast<const f32x4*>(hyper + p * hstride + ch);
    f32x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = (float)s[e] + mu[e];
    *reinterpret_cast<f32x4*>(y_hat + p * c + ch) = o;
  }
}

// ----------------------------- deep factorized -----------------------------
// record holds softplus(matrix), bias, tanh(factor) for one channel
__device__ __forceinline__ float df_logits(const float* __restrict__ rec, const DFDesc& d, float x) {
  float hcur[kMaxW] = {x, 0.f, 0.f, 0.f};
#pragma unroll
  for (int k = 0; k < kMaxL; ++k) {
    if (k < d.nl) {
      const int fi = d.w[k], fo = d.w[k + 1];
      float hn[kMaxW] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int o = 0; o < kMaxW; ++o) {
        if (o < fo) {
          float s = rec[d.off_b[k] + o];
#pragma unroll
          for (int i = 0; i < kMaxW; ++i)
            if (i < fi) s += rec[d.off_m[k] + o * fi + i] * hcur[i];
          if (k < d.nl - 1) s += rec[d.off_f[k] + o] * tanhf(s);
          hn[o] = s;
        }
      }
#pragma unroll
      for (int o = 0; o < kMaxW; ++o) hcur[o] = hn[o];
    }
  }
  return hcur[0];
}

__global__ void __launch_bounds__(256) factorized_kernel(const float* __restrict__ rec_all, DFDesc d, const float* __restrict__ z,
                                                         int64_t hw, int c, float* __restrict__ z_hat,
                                                         double* __restrict__ bits, int values_only) {
  const int img = blockIdx.y;
  const int64_t per = hw * c;
  double acc = 0.0;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < per; i += (int64_t)gridDim.x * blockDim.x) {
    const int ch = (int)(i % c);
    const float zin = z[img * per + i];
    const float v = values_only ? zin : rintf(zin);
    const float* rec = rec_all + (size_t)ch * d.stride;
    const float hi = df_logits(rec, d, v + 0.5f);
    const float lo = df_logits(rec, d, v - 0.5f);
    const bool right = hi > 0.0f;
    const float big = log_sigmoid_f(right ? -lo : hi);
    const float small = log_sigmoid_f(right ? -hi : lo);
    acc += (double)(-log_diff_exp(big, small) * kInvLn2);
    if (!values_only) z_hat[img * per + i] = v;
  }
  block_sum_to(acc, bits + img);
}

// ---- round 6: the same likelihood for the priors the reference actually builds (widths 1 -> W -> ... -> W -> 1, W = 3:
// tfc.NoisyDeepFactorized(num_filters=(3, 3[, 3])), mshyper/models.py:135) with the thread owning a CHANNEL: its record
// (softplus(matrix), bias, tanh(factor): 33 / 48 floats) is read once into registers, then a run of pixels streams past, coalesced
// across the block's channels.  tanh as 1 - 2 / (exp(2 h) + 1) (absolute error 1e-7, scaled by |tanh(factor)| < 1 into the logits),
// and  ln[sigmoid(u) - sigmoid(w)] = ln sigmoid(u) + ln(1 - e^(w - u)) - softplus(w)  with the small arguments of the logarithms
// through their series -- about 250 vector instructions per symbol where the generic kernel above spends ~1500 (tanhf, log1pf,
// expf of the device library, the 64-bit index arithmetic, 33 scattered parameter loads per symbol); VERDICT r5: 57 us of pure
// latency for 4.4 MB on every encode.  Same integers; the bits agree with the float64 oracle as before (test_entropy_factorized).
__device__ __forceinline__ float tanh_fast(float x) {
  return 1.0f - 2.0f * __builtin_amdgcn_rcpf(exp_f(2.0f * x) + 1.0f);
}

__device__ __forceinline__ float ln1p_pos(float t) {      // ln(1 + t), 0 <= t <= 1
  const float ser = t * fmaf(t, fmaf(t, fmaf(t, fmaf(t, 0.2f, -0.25f), 0.33333334f), -0.5f), 1.0f);
  return t < 0.03125f ? ser : logf(1.0f + t);
}

template <int NL, int W>
struct DFRec {
  float m0[W], b0[W], f0[W];                  // 1 -> W
  float mh[NL > 2 ? NL - 2 : 1][W * W], bh[NL > 2 ? NL - 2 : 1][W], fh[NL > 2 ? NL - 2 : 1][W];   // W -> W
  float ml[W], bl;                            // W -> 1
};

template <int NL, int W>
__device__ __forceinline__ float df_logits_fast(const DFRec<NL, W>& r, float x) {
  float hcur[W];
#pragma unroll
  for (int o = 0; o < W; ++o) {
    const float s = r.b0[o] + r.m0[o] * x;
    hcur[o] = s + r.f0[o] * tanh_fast(s);
  }
#pragma unroll
  for (int k = 0; k < NL - 2; ++k) {
    float hn[W];
#pragma unroll
    for (int o = 0; o < W; ++o) {
      float s = r.bh[k][o];
#pragma unroll
      for (int i = 0; i < W; ++i) s += r.mh[k][o * W + i] * hcur[i];
      hn[o] = s + r.fh[k][o] * tanh_fast(s);
    }
#pragma unroll
    for (int o = 0; o < W; ++o) hcur[o] = hn[o];
  }
  float s = r.bl;
#pragma unroll
  for (int i = 0; i < W; ++i) s += r.ml[i] * hcur[i];
  return s;
}

// grid (channel blocks of 256, pixel chunks, n); a thread = one channel, `chunk` consecutive pixels
template <int NL, int W>
__global__ void __launch_bounds__(256) factorized_fast_kernel(const float* __restrict__ rec_all, DFDesc d, const float* __restrict__ z,
                                                              int hw, int c, int chunk, float* __restrict__ z_hat,
                                                              double* __restrict__ bits, int values_only) {
  const int img = blockIdx.z;
  const int ch = blockIdx.x * 256 + threadIdx.x;
  double acc = 0.0;
  if (ch < c) {
    const float* rec = rec_all + (size_t)ch * d.stride;
    DFRec<NL, W> r;
#pragma unroll
    for (int o = 0; o < W; ++o) {
      r.m0[o] = rec[d.off_m[0] + o];
      r.b0[o] = rec[d.off_b[0] + o];
      r.f0[o] = rec[d.off_f[0] + o];
      r.ml[o] = rec[d.off_m[NL - 1] + o];
    }
    r.bl = rec[d.off_b[NL - 1]];
#pragma unroll
    for (int k = 0; k < NL - 2; ++k) {
#pragma unroll
      for (int e = 0; e < W * W; ++e) r.mh[k][e] = rec[d.off_m[k + 1] + e];
#pragma unroll
      for (int o = 0; o < W; ++o) {
        r.bh[k][o] = rec[d.off_b[k + 1] + o];
        r.fh[k][o] = rec[d.off_f[k + 1] + o];
      }
    }
    const int p0 = blockIdx.y * chunk, p1 = min(p0 + chunk, hw);
    const size_t base = (size_t)img * hw * c + ch;
    float b = 0.0f;
    for (int p = p0; p < p1; ++p) {
      const float zin = z[base + (size_t)p * c];
      const float v = values_only ? zin : rintf(zin);
      const float hi = df_logits_fast<NL, W>(r, v + 0.5f);
      const float lo = df_logits_fast<NL, W>(r, v - 0.5f);
      // right of the median the survival pair: P = sigmoid(u) - sigmoid(w), u > w
      const bool right = hi > 0.0f;
      const float u = right ? -lo : hi, w = right ? -hi : lo;
      const float dd = u - w;                                            // > 0: the logits are increasing
      const float e1 = dd * fmaf(dd, fmaf(dd, fmaf(dd, fmaf(dd, 0.0083333338f, -0.041666668f), 0.16666667f), -0.5f), 1.0f);   // 1 - e^-dd, small dd
      const float om = dd < 0.125f ? e1 : 1.0f - exp_f(-dd);
      // ln sigmoid(u) = min(u, 0) - L(u), softplus(w) = max(w, 0) + L(w), L(x) = ln(1 + e^-|x|): no large terms that cancel
      const float lnp = (fminf(u, 0.0f) - fmaxf(w, 0.0f)) + logf(om) - ln1p_pos(exp_f(-fabsf(u))) - ln1p_pos(exp_f(-fabsf(w)));
      b -= fmaf(lnp, 1.925963033500011e-8f, lnp * 1.44269502162933349609375f);
      if (!values_only) z_hat[base + (size_t)p * c] = v;
    }
    acc = (double)b;
  }
  block_sum_to(acc, bits + img);
}

}  // namespace sntc

using namespace sntc;

extern "C" void sntc_prior_destroy(sntc_prior* p) {
  if (!p) return;
  if (p->rec) (void)hipFree(p->rec);
  delete p;
}

extern "C" int sntc_prior_create(int channels, int nlayers, const int* widths, const float* matrices,
                                 const float* biases, const float* factors, void* stream, sntc_prior** prior) {
  if (!widths || !matrices || !biases || !prior || channels < 1)
    return fail(SNTC_ERR_BAD_SHAPE, "sntc_prior_create: null argument");
  if (nlayers < 1 || nlayers > kMaxL) return fail(SNTC_ERR_UNSUPPORTED, "deep factorized: 1..5 affine layers supported");
  if (widths[0] != 1 || widths[nlayers] != 1) return fail(SNTC_ERR_BAD_SHAPE, "deep factorized: widths must start and end with 1");
  for (int k = 0; k <= nlayers; ++k)
    if (widths[k] < 1 || widths[k] > kMaxW) return fail(SNTC_ERR_UNSUPPORTED, "deep factorized: widths up to 4 supported");
  if (nlayers > 1 && !factors) return fail(SNTC_ERR_BAD_SHAPE, "sntc_prior_create: factors missing");
  auto* p = new sntc_prior();
  p->channels = channels;
  DFDesc& d = p->d;
  d.nl = nlayers;
  for (int k = 0; k <= nlayers; ++k) d.w[k] = widths[k];
  int off = 0;
  for (int k = 0; k < nlayers; ++k) {
    d.off_m[k] = off; off += widths[k + 1] * widths[k];
    d.off_b[k] = off; off += widths[k + 1];
    d.off_f[k] = off; off += widths[k + 1];
  }
  d.stride = off;
  std::vector<float> rec((size_t)channels * off, 0.0f);
  size_t pm = 0, pb = 0, pf = 0;
  for (int k = 0; k < nlayers; ++k) {
    const int fi = widths[k], fo = widths[k + 1];
    for (int ch = 0; ch < channels; ++ch) {
      float* r = rec.data() + (size_t)ch * off;
      for (int e = 0; e < fo * fi; ++e) {
        const double m = matrices[pm + (size_t)ch * fo * fi + e];
        r[d.off_m[k] + e] = (float)(m > 30 ? m : std::log1p(std::exp(m)));   // softplus
      }
      for (int e = 0; e < fo; ++e) r[d.off_b[k] + e] = biases[pb + (size_t)ch * fo + e];
      if (k < nlayers - 1)
        for (int e = 0; e < fo; ++e) r[d.off_f[k] + e] = (float)std::tanh((double)factors[pf + (size_t)ch * fo + e]);
    }
    pm += (size_t)channels * fo * fi;
    pb += (size_t)channels * fo;
    if (k < nlayers - 1) pf += (size_t)channels * fo;
  }
  hipError_t e = hipMalloc(&p->rec, rec.size() * sizeof(float));
  if (e != hipSuccess) { delete p; return hip_fail(e, "hipMalloc(prior)"); }
  e = hipMemcpy(p->rec, rec.data(), rec.size() * sizeof(float), hipMemcpyHostToDevice);
  if (e != hipSuccess) { sntc_prior_destroy(p); return hip_fail(e, "hipMemcpy(prior)"); }
  (void)stream;
  *prior = p;
  return SNTC_OK;
}

static int grid_for(int64_t work_items) {
  int64_t b = (work_items + 255) / 256;
  if (b < 1) b = 1;
  if (b > 1024) b = 1024;
  return (int)b;
}

extern "C" int sntc_entropy_factorized(const sntc_prior* prior, const float* z, int n, int64_t hw, float* z_hat,
                                       double* bits, int values_only, void* stream) {
  if (!prior || !z || !bits || (!values_only && !z_hat)) return fail(SNTC_ERR_BAD_SHAPE, "sntc_entropy_factorized: null argument");
  if (n < 1 || hw < 1) return fail(SNTC_ERR_BAD_SHAPE, "sntc_entropy_factorized: empty input");
  hipStream_t s = (hipStream_t)stream;
  if (int zrc = zero_async(bits, sizeof(double) * n, s)) return zrc;
  const int64_t per = hw * prior->channels;
  const DFDesc& d = prior->d;
  bool uniform3 = d.nl >= 3 && d.nl <= 4 && hw < (1 << 30) && n <= 65535;
  for (int k = 1; k < d.nl; ++k) uniform3 = uniform3 && d.w[k] == 3;
  if (uniform3) {
    // a thread = a channel; pixel chunks sized for >= ~4 workgroups per CU's worth of waves without starving a thread of work
    const int cblocks = (prior->channels + 255) / 256;
    int chunk = 8;
    while ((int64_t)cblocks * ((hw + chunk - 1) / chunk) * n > 8192 && chunk < 512) chunk *= 2;
    const dim3 grid(cblocks, (unsigned)((hw + chunk - 1) / chunk), n);
    if (grid.y <= 65535) {
      if (d.nl == 3)
        hipLaunchKernelGGL((factorized_fast_kernel<3, 3>), grid, dim3(256), 0, s, prior->rec, d, z, (int)hw, prior->channels, chunk, z_hat, bits, values_only);
      else
        hipLaunchKernelGGL((factorized_fast_kernel<4, 3>), grid, dim3(256), 0, s, prior->rec, d, z, (int)hw, prior->channels, chunk, z_hat, bits, values_only);
      SNTC_HIP(hipGetLastError());
      return SNTC_OK;
    }
  }
  hipLaunchKernelGGL(factorized_kernel, dim3(grid_for(per), n), dim3(256), 0, s, prior->rec, prior->d, z, hw,
                     prior->channels, z_hat, bits, values_only);
  SNTC_HIP(hipGetLastError());
  return SNTC_OK;
}

extern "C" int sntc_entropy_scale_normal(const float* y, const float* hyper, int n, int64_t hw, int c, float* y_hat,
                                         int32_t* symbols, double* bits, int values_only, void* stream) {
  if (!y || !hyper || !bits || (!values_only && !y_hat)) return fail(SNTC_ERR_BAD_SHAPE, "sntc_entropy_scale_normal: null argument");
  if (n < 1 || hw < 1 || c < 1) return fail(SNTC_ERR_BAD_SHAPE, "sntc_entropy_scale_normal: empty input");
  if (c % 4) return fail(SNTC_ERR_UNSUPPORTED, "sntc_entropy_scale_normal: channels must be a multiple of 4");
  hipStream_t s = (hipStream_t)stream;
  if (int zrc = zero_async(bits, sizeof(double) * n, s)) return zrc;
  // four 16-B vectors per thread: the per-thread costs (set-up, the block reduction, one double atomic per block and image) over
  // 16 symbols, and 12 loads in flight per lane
  const int64_t nvec = hw * (c / 4);
  const int blocks = (int)std::min<int64_t>(std::max<int64_t>((nvec + 1023) / 1024, 1), 1024);
  const int64_t stride = (int64_t)blocks * 256;
  const int dq = (int)(stride / (c / 4)), dr = (int)(stride % (c / 4));
  if (values_only)
    hipLaunchKernelGGL(scale_normal_kernel<true>, dim3(blocks, n), dim3(256), 0, s, y, hyper, hw, c, y_hat, symbols, bits, dq, dr);
  else
    hipLaunchKernelGGL(scale_normal_kernel<false>, dim3(blocks, n), dim3(256), 0, s, y, hyper, hw, c, y_hat, symbols, bits, dq, dr);
  SNTC_HIP(hipGetLastError());
  return SNTC_OK;
}

extern "C" int sntc_dequant_scale_normal(const int32_t* symbols, const float* hyper, int n, int64_t hw, int c,
                                         float* y_hat, void* stream) {
  if (!symbols || !hyper || !y_hat) return fail(SNTC_ERR_BAD_SHAPE, "sntc_dequant_scale_normal: null argument");
  if (n < 1 || hw < 1 || c < 1 || (c % 4)) return fail(SNTC_ERR_BAD_SHAPE, "sntc_dequant_scale_normal: bad sizes");
  const int64_t npix = (int64_t)n * hw;
  hipLaunchKernelGGL(dequant_kernel, dim3(grid_for(npix * c / 4)), dim3(256), 0, (hipStream_t)stream, symbols, hyper,
                     npix, c, 2 * c, y_hat);
  SNTC_HIP(hipGetLastError());
  return SNTC_OK;
}

extern "C" int sntc_dequant_mean(const int32_t* symbols, const float* mu, int n, int64_t hw, int c, int mu_stride, float* y_hat,
                                 void* stream) {
  if (!symbols || !mu || !y_hat) return fail(SNTC_ERR_BAD_SHAPE, "sntc_dequant_mean: null argument");
  if (n < 1 || hw < 1 || c < 1 || (c % 4) || mu_stride < c || (mu_stride % 4))
    return fail(SNTC_ERR_BAD_SHAPE, "sntc_dequant_mean: bad sizes (c % 4 == 0, mu_stride >= c, mu_stride % 4 == 0)");
  const int64_t npix = (int64_t)n * hw;
  hipLaunchKernelGGL(dequant_kernel, dim3(grid_for(npix * c / 4)), dim3(256), 0, (hipStream_t)stream, symbols, mu,
                     npix, c, mu_stride, y_hat);
  SNTC_HIP(hipGetLastError());
  return SNTC_OK;
}
