// rdoq_rules.h -- the decision of rate-distortion optimised quantisation ("RDOQ"; rdoq.hip), one copy: which
// integer an element is coded as, given the argument u = step_scaled(step_diff(y, mu), inv_step) that step_round rounds, its
// nearest integer s0 = step_round(...), the weight w of a squared symbol-unit error in cost_q units and the exact integer price
// of a symbol under the element's own table (cost_q, what sntc_rans_cost sums):
//   candidates, in order   s0;  a = s0 - sign(s0), one towards zero;  0, if flags & kRdoqTryZero and a != 0
//   J(s) = fadd(fmul(w, fmul(e, e)), (float)price(s)),  e = fsub(u, (float)s)      every operation ONE float32 rounding, none fused
//   the smallest J wins; a later candidate replaces an earlier one only on strict <
// A NaN J compares false, so it never displaces s0; a tie keeps the nearer symbol.  s0 is the nearest integer: every other
// candidate has e^2 at least as large, so (w >= 0) a change is always to a strictly cheaper symbol.  s0 == 0 has no candidate.
#pragma once
#include <hip/hip_runtime.h>

namespace sntc {

constexpr int kRdoqTryZero = 1;                             // flags bit 0: also try the symbol 0

__device__ __forceinline__ float rdoq_cost(float u, int s, float w, unsigned price) {
  const float e = __fsub_rn(u, (float)s);
  return __fadd_rn(__fmul_rn(w, __fmul_rn(e, e)), (float)price);
}

// price(s) -> the cost_q entry of the integer s under the element's table
template <class Price>
__device__ __forceinline__ int rdoq_choose(float u, int s0, float w, int flags, Price price) {
  if (s0 == 0) return s0;
  int best = s0;
  float jb = rdoq_cost(u, s0, w, price(s0));
  const int a = s0 - (s0 > 0 ? 1 : -1);
  const float ja = rdoq_cost(u, a, w, price(a));
  if (ja < jb) {
    best = a;
    jb = ja;
  }
  if ((flags & kRdoqTryZero) && a != 0) {
    const float jz = rdoq_cost(u, 0, w, price(0));
    if (jz < jb) best = 0;
  }
  return best;
}

}  // namespace sntc
