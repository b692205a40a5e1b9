// step_rules.h -- the quantisation-step rule of the scale ladder, one device function per half, shared by the
// coder's kernels (quant_step.hip, per image and per latent position) and by SGA iterative inference at a step (sga.hip):
//   symbol    s = (int)rintf((y - mu) * inv_step)            float32 subtract (step_diff), then float32 multiply (step_round)
//   table id  t = clamp(t0 - k, 0, 63)                       step_table_id
//   value     y_hat = fmaf(step, (float)s, mu)               step_value
#pragma once
#include <hip/hip_runtime.h>

namespace sntc {

__device__ __forceinline__ float step_diff(float y, float mu) { return y - mu; }

__device__ __forceinline__ int step_round(float d, float inv_step) { return (int)rintf(d * inv_step); }

__device__ __forceinline__ float step_value(int s, float mu, float step) { return fmaf(step, (float)s, mu); }

// The table-id rule of the coder's kernels (quant_step.hip, per image and per position): the table `shift`
// places down the ladder; off the ladder's ends the end table stays.
constexpr int kLadderTop = 63;                              // last table of the scale ladder (64 normal tables)

__device__ __forceinline__ unsigned step_table_id(unsigned t0, int shift) {
  return (unsigned)min(max((int)t0 - shift, 0), kLadderTop);
}

// The same two halves where the sample is not an integer (SGA at a step): u = step_diff * inv_step is the argument step_round
// rounds, and the value rule on a float v; at an integer u and v = u they are the coder's symbol and step_value of it.
__device__ __forceinline__ float step_scaled(float d, float inv_step) { return d * inv_step; }

__device__ __forceinline__ float step_value_at(float v, float mu, float step) { return fmaf(step, v, mu); }

// A ladder index per latent POSITION (quant_step.hip, the SGA map kernels of sga.hip): the host uploads one table `lut`,
// float32 [2][kMapLut], row 0 = step, row 1 = inv_step, column k - kMapMin; every kernel clamps the byte it reads from a map
// with map_index before it indexes the table, so a stray byte can never read outside it.
constexpr int kMapMin = -32, kMapMax = 32;                  // ladder indexes a map may hold
constexpr int kMapLut = kMapMax - kMapMin + 1;              // entries of a row of the step table: [step | inv_step]

__device__ __forceinline__ int map_index(int k) { return min(max(k, kMapMin), kMapMax); }

}  // namespace sntc
