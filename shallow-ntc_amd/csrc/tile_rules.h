// tile_rules.h -- the geometry of tiled files (wire format 9, DESIGN.md 4.7 "tiled files"), one definition: the kernels of
// tiles.hip include it, any host compiler compiles it into tests/tiles_host.cc, shallow-ntc_amd/tiling.py restates it in Python.
// The reference never writes a file (mshyper/models.py:246-251) and has no tiles.  Everything is per axis and in integers, for a
// length L, a tile size T and an overlap O with T >= 4, T % 4 == 0, 0 <= O <= min(T / 4, 1024) (tile_valid):
//   count     R = max(1, L div T)                                                                  tile_count
//   core      tile r owns [r T, (r + 1) T) for r < R - 1, the last one [(R - 1) T, L): its length lies in [T, 2 T), or is L when
//             R = 1 -- no tile is shorter than min(L, T), so a model's reflect padding (pad < size) holds whenever it holds for T
//   extent    the core grown by O on each interior side: [r T - O, (r + 1) T + O), clipped to [0, L)   tile_begin / tile_end
//   band      the extents of r and r + 1 meet exactly in [(r + 1) T - O, (r + 1) T + O); 2 O <= T / 2 keeps the bands disjoint
//             and inside the picture, so a position lies in one band (two extents) or in none (one extent)       tile_cover
//   weights   at band offset j = p - ((r + 1) T - O), 0 <= j < 2 O: tile r + 1 weighs 2 j + 1, tile r weighs 4 O - (2 j + 1), the
//             axis denominator is 4 O; outside a band the one tile weighs 1 and the denominator is 1.  Every weight >= 1.
//   blend     in 2-D the weight is the product of the axis weights, D = Dy Dx, and an output value is
//             (sum_t w_t v_t + D / 2) div D: exact integers, whatever the order of the sum                      tile_blend
#pragma once

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define SNTC_TILE_FN __host__ __device__ __forceinline__
#else
#define SNTC_TILE_FN inline
#endif

namespace sntc {

constexpr int kTileMin = 4;                                  // T >= 4 and T % 4 == 0: O <= T / 4 is then an integer bound
constexpr int kTileMaxOverlap = 1024;                        // tile_blend stays in 32 bits

SNTC_TILE_FN constexpr bool tile_valid(int L, int T, int O) { return L >= 1 && T >= kTileMin && T % 4 == 0 && O >= 0 && O <= T / 4 && O <= kTileMaxOverlap; }

SNTC_TILE_FN constexpr int tile_count(int L, int T) { return L / T > 1 ? L / T : 1; }

// the extent [tile_begin, tile_end) of tile r of R
SNTC_TILE_FN constexpr int tile_begin(int T, int O, int r) { return r == 0 ? 0 : r * T - O; }
SNTC_TILE_FN constexpr int tile_end(int L, int T, int O, int R, int r) { return r == R - 1 ? L : (r + 1) * T + O; }

// the tiles whose extents hold position p of an axis: tile r with weight w0 and, inside a band (two == 1), tile r + 1 with w1
struct TileCover {
  int r, two, w0, w1, den;
};

// the cover of position p given (k, j) = divmod(p + O, T): the band between tiles k - 1 and k starts at k T - O, j is the offset
// inside it.  A kernel that walks along an axis steps (k, j) instead of dividing again.
SNTC_TILE_FN constexpr TileCover tile_cover_at(int O, int R, int k, int j) {
  if (k >= 1 && k <= R - 1 && j < 2 * O) return TileCover{k - 1, 1, 4 * O - (2 * j + 1), 2 * j + 1, 4 * O};
  const int r = j >= O ? k : k - 1;                          // p div T, p = k T + j - O
  return TileCover{r < R - 1 ? r : R - 1, 0, 1, 0, 1};
}

SNTC_TILE_FN constexpr TileCover tile_cover(int T, int O, int R, int p) {
  const int q = p + O, k = q / T;
  return tile_cover_at(O, R, k, q - k * T);
}

// (sum + D / 2) div D.  The weights of a position sum to D <= (4 O)^2 and v <= 255, so sum + D / 2 < 256 (4 O)^2 <= 2^32 for
// O <= kTileMaxOverlap: unsigned 32-bit arithmetic is exact
SNTC_TILE_FN constexpr unsigned tile_blend(unsigned sum, unsigned den) { return (sum + den / 2u) / den; }

}  // namespace sntc
