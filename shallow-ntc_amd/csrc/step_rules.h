// step_rules.h -- the quantisation-step rule of the scale ladder, one device function per half, shared by the
// coder's kernels (quant_step.hip) and by SGA iterative inference at a step (sga.hip):
//   symbol    s = (int)rintf((y - mu) * inv_step)            float32 subtract (step_diff), then float32 multiply (step_round)
//   value     y_hat = fmaf(step, (float)s, mu)               step_value
#pragma once
#include <hip/hip_runtime.h>

namespace sntc {

__device__ __forceinline__ float step_diff(float y, float mu) { return y - mu; }

__device__ __forceinline__ int step_round(float d, float inv_step) { return (int)rintf(d * inv_step); }

__device__ __forceinline__ float step_value(int s, float mu, float step) { return fmaf(step, (float)s, mu); }

// The same two halves where the sample is not an integer (SGA at a step): u = step_diff * inv_step is the argument step_round
// rounds, and the value rule on a float v; at an integer u and v = u they are the coder's symbol and step_value of it.
__device__ __forceinline__ float step_scaled(float d, float inv_step) { return d * inv_step; }

__device__ __forceinline__ float step_value_at(float v, float mu, float step) { return fmaf(step, v, mu); }

}  // namespace sntc
