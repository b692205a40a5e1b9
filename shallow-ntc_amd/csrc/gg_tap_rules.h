// gg_tap_rules.h -- the byte offset the gather GEMM's vector loader gives one (row, tap) of a tile, two ways:
//   gg_tap_offset_ref   the formula as written down: source pixel, bounds, product -- per row AND per tap
//   gg_tap_row / gg_tap_delta / gg_tap_select / gg_tap_offset
//                       the same offset from per-row state made once per tile (base, mask) and wave-uniform per-tap state
//                       (delta, select word) that the K loop advances with scalar adds: what gather_gemm_kernel.h runs
// Plain functions, compiled by the device compiler into the kernel and by any host compiler into tests/gg_tap_offsets_host.cc,
// which walks both over every (row, tap) of small layers.  An offset with bit 31 set is out of range of the input descriptor
// (buffers are < 2 GiB) and reads zeros; where bit 31 is clear the two rules give the same offset.
#pragma once

#if defined(__HIPCC__)
#define SNTC_TAP_FN __host__ __device__ __forceinline__
#else
#define SNTC_TAP_FN inline
#endif

namespace sntc {

constexpr unsigned kTapOutOfRange = 0x80000000u;
constexpr int kTapGridMax = 16;     // the mask has 16 bits per axis: conv_plan.hip rejects a vector-path tap grid wider or taller

// Layer geometry as GGArgs carries it.  src(row, tap) = (iy0 + ty * tstep, ix0 + tx * tstep) with iy0 = qy * sA + offy.
struct TapGeo {
  int H, W, Cin, sA, tstep, offy, offx;
};

// ---- reference: the offset of tap (ty, tx) for the row (n, qy, qx, valid), 16-B chunk `chunk` of the channel slab
SNTC_TAP_FN unsigned gg_tap_offset_ref(const TapGeo& g, int n, int qy, int qx, int valid, int chunk, int ty, int tx) {
  const unsigned img = valid ? (unsigned)n * (unsigned)(g.H * g.W) * (unsigned)g.Cin * 4u + (unsigned)chunk * 16u : kTapOutOfRange;
  const int iy = qy * g.sA + g.offy + ty * g.tstep;
  const int ix = qx * g.sA + g.offx + tx * g.tstep;
  const bool ok = (unsigned)iy < (unsigned)g.H && (unsigned)ix < (unsigned)g.W;
  const unsigned pix = ((unsigned)(iy * g.W + ix) * (unsigned)g.Cin * 4u) & 0x7fffffffu;
  return (img + pix) | (ok ? 0u : kTapOutOfRange);
}

// ---- per-tile row state.  base: offset of tap (0, 0) mod 2^32 (the tap may lie outside the image: the sum is then never used
// without bit 31).  mask: bit ty = image row iy0 + ty * tstep is inside [0, H), bit 16 + tx = column ix0 + tx * tstep is inside
// [0, W); a padding row has no bit set.
SNTC_TAP_FN void gg_tap_row(const TapGeo& g, int n, int qy, int qx, int valid, int chunk, int th, int tw, unsigned* base,
                            unsigned* mask) {
  const int iy0 = qy * g.sA + g.offy;
  const int ix0 = qx * g.sA + g.offx;
  *base = ((unsigned)n * (unsigned)(g.H * g.W) + (unsigned)(iy0 * g.W + ix0)) * (unsigned)g.Cin * 4u + (unsigned)chunk * 16u;
  unsigned m = 0;
  if (valid) {
    const int tmax = th > tw ? th : tw;       // <= kTapGridMax; wave-uniform, so a 1x1 layer pays for one tap
    for (int t = 0; t < tmax; ++t) {
      if (t < th && (unsigned)(iy0 + t * g.tstep) < (unsigned)g.H) m |= 1u << t;
      if (t < tw && (unsigned)(ix0 + t * g.tstep) < (unsigned)g.W) m |= 0x10000u << t;
    }
  }
  *mask = m;
}

// ---- per-tap state, the same for every row of the launch
SNTC_TAP_FN unsigned gg_tap_dx(const TapGeo& g) { return (unsigned)g.tstep * (unsigned)g.Cin * 4u; }                   // tx -> tx + 1
SNTC_TAP_FN unsigned gg_tap_dy(const TapGeo& g) { return (unsigned)(g.tstep * g.W) * (unsigned)g.Cin * 4u; }           // ty -> ty + 1
SNTC_TAP_FN unsigned gg_tap_delta(const TapGeo& g, int ty, int tx) { return (unsigned)ty * gg_tap_dy(g) + (unsigned)tx * gg_tap_dx(g); }
SNTC_TAP_FN unsigned gg_tap_select(int ty, int tx) { return (1u << ty) | (0x10000u << tx); }

// ---- the loop's per-row work: one add, one and, one compare, one select-or
SNTC_TAP_FN unsigned gg_tap_offset(unsigned base, unsigned mask, unsigned delta, unsigned select) {
  const unsigned off = base + delta;
  return (mask & select) == select ? off : (off | kTapOutOfRange);
}

}  // namespace sntc
