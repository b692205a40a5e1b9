// tiles_host.cc -- a stand-alone host program over csrc/tile_rules.h, the header the kernels of csrc/tiles.hip compile: for every
// (L, T, O) on its command line (three ints each) it checks the rule's own promises and prints the tables
// tests/test_tiling_host.py compares with the Python mirror (shallow-ntc_amd/tiling.py):
//   axis L T O R
//   tile r begin end                       the extent of every tile
//   pos p r two w0 w1 den                  tile_cover of every position
// Checked here, counted as mismatches: every position lies in the extents of exactly the tiles its cover names, the weights are
// >= 1 and sum to the denominator, the two weights of a band position are those of the band offset, no extent is shorter than
// min(L, T), and tile_blend of equal values returns the value.
#include <cstdio>
#include <cstdlib>

#include "../shallow-ntc_amd/csrc/tile_rules.h"

using namespace sntc;

static_assert(tile_count(15, 8) == 1 && tile_count(16, 8) == 2 && tile_count(17, 8) == 2 && tile_count(5, 8) == 1, "tile_count");
static_assert(tile_end(17, 8, 2, 2, 1) == 17 && tile_begin(8, 2, 1) == 6 && tile_end(17, 8, 2, 2, 0) == 10, "extents");
static_assert(tile_cover(8, 2, 2, 6).two == 1 && tile_cover(8, 2, 2, 6).w1 == 1 && tile_cover(8, 2, 2, 6).w0 == 7, "band start");
static_assert(tile_cover(8, 2, 2, 9).w1 == 7 && tile_cover(8, 2, 2, 10).two == 0 && tile_cover(8, 2, 2, 10).r == 1, "band end");
static_assert(tile_blend(255u * 16777216u, 16777216u) == 255u, "tile_blend at the largest denominator");

int main(int argc, char** argv) {
  if (argc < 4 || (argc - 1) % 3) {
    std::fprintf(stderr, "usage: tiles_host L T O [L T O ...]\n");
    return 2;
  }
  long mismatches = 0, walked = 0;
  for (int a = 1; a + 2 < argc; a += 3) {
    const int L = std::atoi(argv[a]), T = std::atoi(argv[a + 1]), O = std::atoi(argv[a + 2]);
    if (!tile_valid(L, T, O)) {
      std::printf("invalid %d %d %d\n", L, T, O);
      continue;
    }
    const int R = tile_count(L, T);
    std::printf("axis %d %d %d %d\n", L, T, O, R);
    for (int r = 0; r < R; ++r) {
      const int b = tile_begin(T, O, r), e = tile_end(L, T, O, R, r);
      std::printf("tile %d %d %d\n", r, b, e);
      if (b < 0 || e > L || e - b < (L < T ? L : T)) ++mismatches;
    }
    for (int p = 0; p < L; ++p) {
      const TileCover c = tile_cover(T, O, R, p);
      std::printf("pos %d %d %d %d %d %d\n", p, c.r, c.two, c.w0, c.w1, c.den);
      for (int r = 0; r < R; ++r) {
        const bool in = tile_begin(T, O, r) <= p && p < tile_end(L, T, O, R, r);
        const bool named = r == c.r || (c.two && r == c.r + 1);
        if (in != named) ++mismatches;
      }
      if (c.w0 < 1 || (c.two ? c.w1 < 1 : c.w1 != 0) || c.w0 + c.w1 != c.den || c.den != (c.two ? 4 * O : 1)) ++mismatches;
      if (c.two) {
        const int j = p - ((c.r + 1) * T - O);
        if (j < 0 || j >= 2 * O || c.w1 != 2 * j + 1) ++mismatches;
      }
      for (unsigned v = 0; v < 256; v += 51)
        if (tile_blend(v * (unsigned)c.den * (unsigned)c.den, (unsigned)c.den * (unsigned)c.den) != v) ++mismatches;
      ++walked;
    }
  }
  std::printf("walked %ld positions, %ld mismatches\n", walked, mismatches);
  return mismatches ? 1 : 0;
}
