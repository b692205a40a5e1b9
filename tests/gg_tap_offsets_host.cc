// gg_tap_offsets_host.cc -- stand-alone check of csrc/gg_tap_rules.h (built and run by tests/test_gg_tap_offsets_host.py):
// for every (row, tap) of small layers the per-tile state rule (base + delta, mask & select) must give the reference formula's
// byte offset wherever that is in range, and bit 31 wherever the reference has it.  The tap walk is the kernel's: started at
// an arbitrary stage of the tile and advanced with adds, the delta reset at the end of a channel slab.
//
// Geometry as csrc/conv_plan.hip sets it (geometry(), build_plan()):
//   forward k x k / s, SAME:  Ho = ceil(h / s), pt = max((Ho - 1) s + k - h, 0) / 2;  Q = (Ho, Wo), sA = s, tstep = 1, off = -pad
//   transposed k x k / s:     pad = max(k - s, 0) / 2, phases grouped per axis by tap count cnt(phi) = (k - phi + s - 1) / s,
//                             q0(phi) = phi < pad;  sA = 1, tstep = -1, off = 0 (s = 1: one group, off = +pad);  exact grid (every class has one q0): Q = (h, w) and
//                             the group's origin q0, otherwise Q = ((h s - 1 + pad) / s + 1, ...) and origin 0
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../shallow-ntc_amd/csrc/gg_tap_rules.h"

using namespace sntc;

struct Group { int th, tw, q0y, q0x; };
struct Layer { TapGeo g; int Qh, Qw; std::vector<Group> groups; };

static long long g_checked = 0, g_in_range = 0, g_failed = 0;

static Layer forward_layer(int k, int s, int h, int w, int cin) {
  const int Ho = (h + s - 1) / s, Wo = (w + s - 1) / s;
  const int pt = std::max((Ho - 1) * s + k - h, 0) / 2, pl = std::max((Wo - 1) * s + k - w, 0) / 2;
  return Layer{TapGeo{h, w, cin, s, 1, -pt, -pl}, Ho, Wo, {Group{k, k, 0, 0}}};
}

static Layer transposed_layer(int k, int s, int h, int w, int cin) {
  const int pad = std::max(k - s, 0) / 2;
  if (s == 1)      // stride 1: correlation with the flipped kernel, one group
    return Layer{TapGeo{h, w, cin, 1, -1, pad, pad}, h, w, {Group{k, k, 0, 0}}};
  struct Cls { int cnt, q0; bool uniform; };
  std::vector<Cls> cls;
  for (int phi = 0; phi < s; ++phi) {
    const int cnt = (k - phi + s - 1) / s, q0 = phi < pad ? 1 : 0;
    bool found = false;
    for (auto& c : cls)
      if (c.cnt == cnt) { c.uniform = c.uniform && c.q0 == q0; found = true; }
    if (!found) cls.push_back(Cls{cnt, q0, true});
  }
  bool exact = pad < s;
  for (auto& c : cls) exact = exact && c.uniform;
  Layer L{TapGeo{h, w, cin, 1, -1, 0, 0}, exact ? h : (h * s - 1 + pad) / s + 1, exact ? w : (w * s - 1 + pad) / s + 1, {}};
  for (auto& a : cls)
    for (auto& b : cls) L.groups.push_back(Group{a.cnt, b.cnt, exact ? a.q0 : 0, exact ? b.q0 : 0});
  return L;
}

// one tile of BM rows starting at row m0 of the launch's M = n * Qh * Qw rows, as write_rinfo / init_loader / advance_stage do
static void check_tile(const Layer& L, const Group& G, int nimg, int m0, int BM, int slabs, int k0) {
  const int M = nimg * L.Qh * L.Qw, T = G.th * G.tw;
  const unsigned dx = gg_tap_dx(L.g), drow = gg_tap_dy(L.g) - (unsigned)(G.tw - 1) * dx;
  for (int r = 0; r < BM; ++r) {
    const int m = m0 + r;
    int n = 0, qy = 0, qx = 0, valid = 0;
    if (m < M) {
      const int per = L.Qh * L.Qw;
      n = m / per;
      const int rem = m - n * per;
      qy = rem / L.Qw + G.q0y;
      qx = rem - (rem / L.Qw) * L.Qw + G.q0x;
      valid = 1;
    }
    for (int chunk = 0; chunk < 4; ++chunk) {
      unsigned base, mask;
      gg_tap_row(L.g, n, qy, qx, valid, chunk, G.th, G.tw, &base, &mask);
      // the loader's walk from stage k0 (slab-outermost: stage = cc * T + t)
      int t = k0 % T, ty = t / G.tw, tx = t % G.tw;
      unsigned delta = gg_tap_delta(L.g, ty, tx), sel = gg_tap_select(ty, tx);
      for (int stage = k0; stage < slabs * T; ++stage) {
        const unsigned ref = gg_tap_offset_ref(L.g, n, qy, qx, valid, chunk, ty, tx);
        const unsigned got = gg_tap_offset(base, mask, delta, sel);
        ++g_checked;
        bool ok;
        if (ref & kTapOutOfRange) {
          ok = (got & kTapOutOfRange) != 0;
        } else {
          ok = got == ref;
          ++g_in_range;
          // an in-range offset addresses this row's own pixel: inside the n-th image of an (nimg, H, W, Cin) tensor
          const unsigned img_bytes = (unsigned)(L.g.H * L.g.W * L.g.Cin * 4);
          ok = ok && ref >= (unsigned)n * img_bytes && ref + 16 <= (unsigned)(n + 1) * img_bytes;
        }
        if (!ok && ++g_failed <= 10)
          std::fprintf(stderr, "MISMATCH H=%d W=%d Cin=%d sA=%d tstep=%d off=(%d,%d) row=(%d,%d,%d,%d) chunk=%d tap=(%d,%d): ref %08x got %08x\n",
                       L.g.H, L.g.W, L.g.Cin, L.g.sA, L.g.tstep, L.g.offy, L.g.offx, n, qy, qx, valid, chunk, ty, tx, ref, got);
        // advance_stage
        const bool row_end = tx + 1 == G.tw, tap_end = t + 1 == T;
        tx = row_end ? 0 : tx + 1;
        ty = tap_end ? 0 : ty + (row_end ? 1 : 0);
        t = tap_end ? 0 : t + 1;
        delta = tap_end ? 0u : delta + (row_end ? drow : dx);
        sel = gg_tap_select(ty, tx);
      }
    }
  }
}

static void check_layer(const Layer& L, int nimg) {
  const int M = nimg * L.Qh * L.Qw;
  for (const Group& G : L.groups) {
    if (G.th > kTapGridMax || G.tw > kTapGridMax) { std::fprintf(stderr, "tap grid beyond the masks\n"); std::exit(2); }
    for (int BM : {64, 128}) {                              // M is rarely a multiple of the tile: the last tile has padding rows
      const int slabs = L.g.Cin / 16, T = G.th * G.tw;
      for (int m0 = 0; m0 < M; m0 += BM) {
        check_tile(L, G, nimg, m0, BM, slabs, 0);
        check_tile(L, G, nimg, m0, BM, slabs, (m0 / BM * 7 + 3) % (slabs * T));   // a stream-K tail piece: starts inside a tile
      }
    }
  }
}

int main() {
  const int sizes[][2] = {{1, 1}, {1, 4}, {2, 3}, {3, 1}, {4, 6}, {5, 7}, {8, 8}, {9, 11}};
  for (auto& hw : sizes)
    for (int nimg = 1; nimg <= 3; ++nimg) {
      for (int k : {1, 3, 5})
        for (int s : {1, 2}) check_layer(forward_layer(k, s, hw[0], hw[1], 32), nimg);
      check_layer(transposed_layer(5, 2, hw[0], hw[1], 32), nimg);
      check_layer(transposed_layer(13, 8, hw[0], hw[1], 16), nimg);
      check_layer(transposed_layer(3, 1, hw[0], hw[1], 32), nimg);   // stride 1: one group, tstep = -1, off = +pad
    }
  // 9 x 11 x 3 images is M = 297: tiles of 64 and 128 rows with one to three images inside and a ragged last tile; the larger
  // batch puts whole images between tile starts
  check_layer(forward_layer(3, 1, 9, 11, 48), 7);
  std::printf("checked %lld (row, tap) offsets, %lld in range, %lld mismatches\n", g_checked, g_in_range, g_failed);
  return g_failed == 0 && g_in_range > 0 ? 0 : 1;
}
