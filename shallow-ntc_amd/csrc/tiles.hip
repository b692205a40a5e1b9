// tiles.hip -- the two pixel-end kernels of tiled files (wire format 9, DESIGN.md 4.7 "tiled files"): a picture is cut into
// overlapping tiles that are coded as the images of ordinary batches, and decoded tiles are put back together with blended seams.
// The reference never writes a file (mshyper/models.py:246-251: compression=False) and knows no tiles; the geometry is
// tile_rules.h, used by the kernels here, by tests/tiles_host.cc and restated in shallow-ntc_amd/tiling.py.
//   tiles_extract_kernel    x float [n][H][W][c], rects (image, y0, x0) -> out [ntiles][th][tw][c]: the tiles of ONE shape class.
//                           Grid (workgroups per tile, tiles); the rects travel in the kernel arguments (a wave-uniform index,
//                           scalar loads).  A thread's unit is V consecutive floats of a tile row: V = 4 (16-byte loads and
//                           stores) where the rows of both sides are 16-byte aligned -- W c, tw c and every x0 c multiples of 4,
//                           both pointers aligned --, V = 1 (coalesced dwords) otherwise: rows of tw 3 floats are not aligned in
//                           general.  One 32-bit division per unit.
//   tiles_assemble_kernel   the window [ry, ry + rh) x [rx, rx + rw) of the picture as a GATHER: every output value is written
//                           once, from the 1, 2 or 4 tiles whose extents hold its pixel (tile_cover per axis), read through a
//                           table of tile pointers -- tiles of different shape classes live in different tensors -- and blended
//                           in integers (tile_blend).  No atomics on pixels and no accumulator: the result does not depend on
//                           the launch.  Grid (workgroups per window row, rows, images).  A thread's unit is one ALIGNED dword of
//                           an output row, so a wave stores 256 contiguous bytes, two whole lines; the up to three bytes in
//                           front of a row's first aligned dword and behind its last go out as byte stores (a row of rw 3 bytes
//                           starts anywhere; the neighbouring row writes its own bytes of a shared dword).  The row's cover is
//                           wave-uniform, the column's costs one 32-bit division per thread and steps from pixel to pixel, and
//                           only a value inside a band pays the blend's division.  It does NOT reach a copy's rate: 7 x the time
//                           of a device copy of its output at 4096 x 4096, cause not found (DESIGN.md 4.7 has the figures).  A
//                           pixel that needs a tile whose pointer is null is written as 0 and counted in `missing` (one integer
//                           atomic per wave that saw any).
#include <algorithm>
#include "sntc_internal.h"
#include "tile_rules.h"

namespace sntc {

constexpr int kTileThreads = 256;
constexpr int kTileRects = 256;                             // rects of one extract launch: 3 KB of kernel arguments
constexpr int kTileGrid = 2048;                             // workgroups of an extract launch, about: eight per CU

struct TileRects {
  int v[kTileRects][3];                                     // image, y0, x0
};

template <int V>
__global__ void __launch_bounds__(kTileThreads) tiles_extract_kernel(const float* __restrict__ x, unsigned H, unsigned W, unsigned c,
                                                                     const TileRects rects, unsigned th, unsigned tw,
                                                                     float* __restrict__ out) {
  const unsigned rowlen = tw * c, E = th * rowlen, nunit = E / V;        // V == 4: rowlen % 4 == 0 (host)
  const unsigned img = (unsigned)rects.v[blockIdx.y][0], y0 = (unsigned)rects.v[blockIdx.y][1], x0 = (unsigned)rects.v[blockIdx.y][2];
  const size_t wc = (size_t)W * c;
  const float* src = x + ((size_t)img * H + y0) * wc + (size_t)x0 * c;
  float* dst = out + (size_t)blockIdx.y * E;
  const unsigned stride = gridDim.x * kTileThreads;
  for (unsigned u = blockIdx.x * kTileThreads + threadIdx.x; u < nunit; u += stride) {
    const unsigned e0 = u * V, row = e0 / rowlen, col = e0 - row * rowlen;
    if constexpr (V == 4) {
      *reinterpret_cast<float4*>(dst + e0) = *reinterpret_cast<const float4*>(src + row * wc + col);
    } else {
      dst[e0] = src[row * wc + col];
    }
  }
}

// what the assemble kernel knows about one axis position: its cover and, per covering tile, where the tile starts and how long
// it is
struct TileAxis {
  TileCover cv;
  int begin[2], len[2];
};

__device__ __forceinline__ TileAxis tile_axis_of(const TileCover& cv, int L, int T, int O, int R) {
  TileAxis a;
  a.cv = cv;
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int r = cv.r + i < R ? cv.r + i : R - 1;          // (i == 1 outside a band: unused)
    a.begin[i] = tile_begin(T, O, r);
    a.len[i] = tile_end(L, T, O, R, r) - a.begin[i];
  }
  return a;
}

// value `ch` of picture pixel (y, x) of one image: `tiles` = the image's R x C pointers.  Outside the bands the one weight and
// the denominator are 1: no division.
template <int CH>
__device__ __forceinline__ unsigned tile_value(const unsigned char* const* __restrict__ tiles, int C, const TileAxis& ay,
                                               const TileAxis& ax, int y, int x, int ch, bool& miss) {
  unsigned sum = 0;
  miss = false;
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    if (i > ay.cv.two) continue;
    const unsigned wy = i ? ay.cv.w1 : ay.cv.w0;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      if (j > ax.cv.two) continue;
      const unsigned wx = j ? ax.cv.w1 : ax.cv.w0;
      const unsigned char* t = tiles[(ay.cv.r + i) * C + ax.cv.r + j];
      if (!t) {
        miss = true;
        continue;
      }
      sum += wy * wx * (unsigned)t[((size_t)(y - ay.begin[i]) * ax.len[j] + (x - ax.begin[j])) * CH + ch];
    }
  }
  if (miss) return 0u;
  return (ay.cv.two | ax.cv.two) ? tile_blend(sum, (unsigned)(ay.cv.den * ax.cv.den)) : sum;
}

// Grid (workgroups per window row, window rows -- strided where there are more than the grid holds --, images); CH = the channel
// count, at compile time: the column of a unit's first value is a division by a constant.  The row's cover is wave-uniform; the
// column's costs ONE division by T per thread, (k, j) = divmod(x + O, T), and steps from pixel to pixel (tile_cover_at).
template <int CH>
__global__ void __launch_bounds__(kTileThreads) tiles_assemble_kernel(const unsigned char* const* __restrict__ tile_ptrs, int H, int W,
                                                                      int T, int O, int R, int C, int ry, int rx, int rh, int rw,
                                                                      unsigned char* __restrict__ out, int* __restrict__ missing) {
  const unsigned rowlen = (unsigned)rw * CH;
  const unsigned char* const* tiles = tile_ptrs + (size_t)blockIdx.z * R * C;
  const unsigned u = blockIdx.x * blockDim.x + threadIdx.x;
  int nmiss = 0;
  for (unsigned row = blockIdx.y; row < (unsigned)rh; row += gridDim.y) {
    unsigned char* orow = out + ((size_t)blockIdx.z * rh + row) * rowlen;
    const unsigned lo = (unsigned)(reinterpret_cast<uintptr_t>(orow) & 3u);        // the row starts `lo` bytes into an aligned dword
    if (u >= (lo + rowlen + 3u) / 4u) continue;
    const int y = ry + (int)row;
    const TileAxis ay = tile_axis_of(tile_cover(T, O, R, y), H, T, O, R);
    const unsigned v0 = 4u * u;                              // the unit's bytes: row values v0 + b - lo, b = 0 .. 3
    const unsigned first = v0 < lo ? 0u : v0 - lo, last = min(v0 + 4u - lo, rowlen);   // [first, last) of the row
    const unsigned col = first / CH;
    unsigned ch = first - col * CH;
    int x = rx + (int)col, k = (x + O) / T, j = x + O - k * T;
    unsigned char val[4] = {0, 0, 0, 0};
    if (last - first == 4u && !ay.cv.two) {
      // The common unit -- a whole dword of a row outside the bands: straight-line code without a branch between its loads, so
      // the four pointer loads can go out together and the four byte loads behind them.  A missing tile's value is read from
      // the pointer table instead (any valid address) and replaced by 0.  (Measured: it did not move the launch's time,
      // DESIGN.md 4.7; kept because it is the shorter path for nine units in ten.)
      const unsigned char* tp[4];
      size_t at[4];
      bool head[4], band = false;
#pragma unroll
      for (unsigned b = 0; b < 4; ++b) {
        const unsigned cb = (first + b) / CH, d = cb - col;               // d <= 3 < T
        int jb = j + (int)d, kb = k;
        if (jb >= T) {
          jb -= T;
          ++kb;
        }
        const TileCover cv = tile_cover_at(O, C, kb, jb);
        band = band || cv.two;
        const int begin = tile_begin(T, O, cv.r), len = tile_end(W, T, O, C, cv.r) - begin;
        tp[b] = tiles[ay.cv.r * C + cv.r];
        at[b] = ((size_t)(y - ay.begin[0]) * len + (rx + (int)cb - begin)) * CH + (first + b - cb * CH);
        head[b] = first + b == cb * CH;
      }
      if (!band) {
#pragma unroll
        for (unsigned b = 0; b < 4; ++b) {
          const unsigned char v = *(tp[b] ? tp[b] + at[b] : reinterpret_cast<const unsigned char*>(tiles));
          val[b] = tp[b] ? v : (unsigned char)0;
          nmiss += (!tp[b] && head[b]) ? 1 : 0;
        }
        *reinterpret_cast<uchar4*>(orow + first) = make_uchar4(val[0], val[1], val[2], val[3]);
        continue;
      }
    }
    TileAxis ax = tile_axis_of(tile_cover_at(O, C, k, j), W, T, O, C);
    for (unsigned e = first; e < last; ++e) {
      bool miss;
      val[e + lo - v0] = (unsigned char)tile_value<CH>(tiles, C, ay, ax, y, x, (int)ch, miss);
      nmiss += (miss && ch == 0) ? 1 : 0;                    // a pixel counts once, with its first value
      if (++ch == CH) {
        ch = 0;
        ++x;
        if (++j == T) {
          j = 0;
          ++k;
        }
        if (e + 1 < last) ax = tile_axis_of(tile_cover_at(O, C, k, j), W, T, O, C);
      }
    }
    if (last - first == 4u) {                                // a whole aligned dword
      *reinterpret_cast<uchar4*>(orow + first) = make_uchar4(val[0], val[1], val[2], val[3]);
    } else {
      for (unsigned e = first; e < last; ++e) orow[e] = val[e + lo - v0];
    }
  }
  for (int off = 32; off > 0; off >>= 1) nmiss += __shfl_down(nmiss, off);
  if ((threadIdx.x & 63) == 0 && nmiss) atomicAdd(missing, nmiss);
}

static inline bool tile_aligned(const void* p, uintptr_t a) { return reinterpret_cast<uintptr_t>(p) % a == 0; }

}  // namespace sntc

using namespace sntc;

extern "C" int sntc_tiles_extract(const float* x, int n, int H, int W, int c, const int32_t* rects, int ntiles, int th, int tw,
                                  float* out, void* stream) {
  if (!x || !rects || !out) return fail(SNTC_ERR_BAD_SHAPE, "sntc_tiles_extract: null argument");
  if (n < 1 || H < 1 || W < 1 || c < 1 || ntiles < 1 || th < 1 || tw < 1 || th > H || tw > W)
    return fail(SNTC_ERR_BAD_SHAPE, "sntc_tiles_extract: bad sizes (n, H, W, c, ntiles >= 1, 1 <= th <= H, 1 <= tw <= W)");
  const int64_t E = (int64_t)th * tw * c;
  if (E > 0x7fffffffLL || (int64_t)W * c > 0x7fffffffLL) return fail(SNTC_ERR_BAD_SHAPE, "sntc_tiles_extract: a tile holds at most 2^31 - 1 values");
  if (!tile_aligned(x, 4) || !tile_aligned(out, 4)) return fail(SNTC_ERR_BAD_SHAPE, "sntc_tiles_extract: misaligned argument");
  bool vec = (tw * (int64_t)c) % 4 == 0 && ((int64_t)W * c) % 4 == 0 && tile_aligned(x, 16) && tile_aligned(out, 16);
  for (int t = 0; t < ntiles; ++t) {
    const int32_t* r = rects + 3 * (size_t)t;
    if (r[0] < 0 || r[0] >= n || r[1] < 0 || r[1] > H - th || r[2] < 0 || r[2] > W - tw)
      return fail(SNTC_ERR_BAD_SHAPE, "sntc_tiles_extract: rect " + std::to_string(t) + " (image " + std::to_string(r[0]) + ", y0 " +
                                          std::to_string(r[1]) + ", x0 " + std::to_string(r[2]) + ") leaves the image");
    vec = vec && ((int64_t)r[2] * c) % 4 == 0;
  }
  const int64_t nunit = vec ? E / 4 : E;
  for (int t0 = 0; t0 < ntiles; t0 += kTileRects) {          // the rects travel as kernel arguments, kTileRects per launch
    const int cnt = std::min(kTileRects, ntiles - t0);
    TileRects tr;
    std::fill(&tr.v[0][0], &tr.v[0][0] + 3 * kTileRects, 0);
    std::copy(rects + 3 * (size_t)t0, rects + 3 * (size_t)(t0 + cnt), &tr.v[0][0]);
    const int64_t want = (nunit + kTileThreads - 1) / kTileThreads, most = std::max<int64_t>(1, kTileGrid / cnt);
    const dim3 grid((unsigned)std::max<int64_t>(1, std::min(want, most)), (unsigned)cnt);
    const auto kernel = vec ? tiles_extract_kernel<4> : tiles_extract_kernel<1>;
    hipLaunchKernelGGL(kernel, grid, dim3(kTileThreads), 0, (hipStream_t)stream, x, (unsigned)H, (unsigned)W, (unsigned)c, tr,
                       (unsigned)th, (unsigned)tw, out + (size_t)t0 * E);
    SNTC_HIP(hipGetLastError());
  }
  return SNTC_OK;
}

extern "C" int sntc_tiles_assemble(const uint8_t* const* tile_ptrs, int n, int H, int W, int c, int tile, int overlap, int ry, int rx,
                                   int rh, int rw, uint8_t* out, int32_t* missing, void* stream) {
  if (!tile_ptrs || !out || !missing) return fail(SNTC_ERR_BAD_SHAPE, "sntc_tiles_assemble: null argument");
  if (n < 1 || n > 65535 || H < 1 || W < 1 || c < 1 || c > 4)
    return fail(SNTC_ERR_BAD_SHAPE, "sntc_tiles_assemble: bad sizes (1 <= n <= 65535, H, W >= 1, 1 <= c <= 4)");
  if (!tile_valid(H, tile, overlap) || !tile_valid(W, tile, overlap))
    return fail(SNTC_ERR_BAD_SHAPE, "sntc_tiles_assemble: tile >= 4, tile % 4 == 0, 0 <= overlap <= min(tile / 4, 1024)");
  if (ry < 0 || rx < 0 || rh < 1 || rw < 1 || ry > H - rh || rx > W - rw)
    return fail(SNTC_ERR_BAD_SHAPE, "sntc_tiles_assemble: the window leaves the picture");
  if ((int64_t)rw * c > 0x7fffffffLL) return fail(SNTC_ERR_BAD_SHAPE, "sntc_tiles_assemble: a window row holds at most 2^31 - 1 values");
  if (!tile_aligned(tile_ptrs, 8) || !tile_aligned(missing, 4)) return fail(SNTC_ERR_BAD_SHAPE, "sntc_tiles_assemble: misaligned argument");
  hipStream_t s = (hipStream_t)stream;
  if (int zrc = zero_async(missing, sizeof(int32_t), s)) return zrc;
  const int64_t nunit = ((int64_t)rw * c + 3 + 3) / 4;       // a row's aligned dwords, at the most
  const int threads = nunit >= kTileThreads ? kTileThreads : 64;       // short rows (a small window): one wave per workgroup
  const dim3 grid((unsigned)((nunit + threads - 1) / threads), (unsigned)std::min(rh, 65535), (unsigned)n);
  const auto kernel = c == 1 ? tiles_assemble_kernel<1> : c == 2 ? tiles_assemble_kernel<2> : c == 3 ? tiles_assemble_kernel<3>
                                                                                                 : tiles_assemble_kernel<4>;
  hipLaunchKernelGGL(kernel, grid, dim3(threads), 0, s, tile_ptrs, H, W, tile, overlap, tile_count(H, tile), tile_count(W, tile), ry, rx,
                     rh, rw, out, missing);
  SNTC_HIP(hipGetLastError());
  return SNTC_OK;
}
