// gg_pieces_host.cc -- stand-alone check of the piece walk in csrc/gg_pieces.h, Part A (built and run by
// tests/test_gg_pieces_host.py): the functions gg_kernel and bf3_kernel run, compiled for the host and walked over every worker
// of small launches.
//
// Stream-K, per geometry, unit order and worker count:
//   1. the reference is the units enumerated by plain nested loops in the documented order (strip-major: mt, group, nt, k;
//      column-major: group, nt, mt, k); the pieces of all workers cover every (tile, k) exactly once, each inside its worker's
//      share, and tile_of(t) is the tile locate named;
//   2. every published piece of worker w has exactly one partner: a piece of worker w + 1 on the same tile with consume == w and
//      k0 == the publisher's k1; no tile is touched by more than two workers;
//   3. worker 0 never consumes;
//   4. no worker emits a consuming piece before its publishing piece, and its head and tail are different tiles;
//   5. a worker with an empty share emits no piece.
// 2 to 4 together are the no-deadlock argument: a worker waits only for worker w - 1, and what it waits for is the FIRST thing
// w - 1 computes, which itself waits for nothing -- so no chain of waits exists, whatever order the hardware dispatches in
// (a worker that is not resident at all is the bounded spin's case, sk_consume).  ("Worker" is the slot wl of worker_slot: the
// workgroups of one XCD own a contiguous eighth of the range.)
// Static, per geometry and ksplit:
//   6. blocks 0 .. tiles * ksplit - 1 map one-to-one onto (group, mt, nt, split);
//   7. the K ranges of a tile partition [0, steps);
//   8. with one group the general column-major rule is the formula gg_kernel's COLM twin had for itself (colm_reference below).
//
// The launch fields tile0 / unit0 / tps / ups / units / blk0 are the host's (work_of and conv_forward_impl in csrc/conv_plan.hip,
// which need the plan and the instance table); fill() restates those five lines.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../shallow-ntc_amd/csrc/gg_pieces.h"

using namespace sntc;

struct HostGroup { int steps, tile0, ntn, blk0; long long unit0; };
struct HostArgs {
  int sk, ngroups, ntm, tps, ups, nworkers, ksplit, order;
  long long units;
  HostGroup g[kPieceGroups];
};

static long long g_geometries = 0, g_walks = 0, g_pieces = 0, g_failed = 0;
static const HostArgs* g_now = nullptr;
static int g_order_now = 0;

static void fail(const char* what, int x = 0, int y = 0) {
  if (++g_failed > 10) return;
  const HostArgs& a = *g_now;
  std::fprintf(stderr, "MISMATCH %s (%d, %d): ngroups=%d ntm=%d nworkers=%d ksplit=%d order=%d steps/ntn =", what, x, y, a.ngroups, a.ntm,
               a.nworkers, a.ksplit, g_order_now);
  for (int i = 0; i < a.ngroups; ++i) std::fprintf(stderr, " %d/%d", a.g[i].steps, a.g[i].ntn);
  std::fprintf(stderr, "\n");
}

// work_of / conv_forward_impl, restated
static void fill(HostArgs& a) {
  a.tps = 0; a.ups = 0;
  int nb = 0;
  for (int gi = 0; gi < a.ngroups; ++gi) {
    a.g[gi].tile0 = a.tps;
    a.g[gi].unit0 = a.ups;
    a.tps += a.g[gi].ntn;
    a.ups += a.g[gi].ntn * a.g[gi].steps;
    a.g[gi].blk0 = nb;
    nb += a.g[gi].ntn * a.ntm * a.ksplit;
  }
  a.units = (long long)a.ups * a.ntm;
}

struct Unit { int gi, mt, nt, k; };

static std::vector<Unit> reference_units(const HostArgs& a, bool strip) {
  std::vector<Unit> ref;
  if (strip) {
    for (int mt = 0; mt < a.ntm; ++mt)
      for (int gi = 0; gi < a.ngroups; ++gi)
        for (int nt = 0; nt < a.g[gi].ntn; ++nt)
          for (int k = 0; k < a.g[gi].steps; ++k) ref.push_back(Unit{gi, mt, nt, k});
  } else {
    for (int gi = 0; gi < a.ngroups; ++gi)
      for (int nt = 0; nt < a.g[gi].ntn; ++nt)
        for (int mt = 0; mt < a.ntm; ++mt)
          for (int k = 0; k < a.g[gi].steps; ++k) ref.push_back(Unit{gi, mt, nt, k});
  }
  return ref;
}

static int tile_index(const HostArgs& a, int gi, int mt, int nt) { return mt * a.tps + a.g[gi].tile0 + nt; }   // a dense key, any order

// 8: what gg_kernel's COLM twin computed for its single group before the rule was shared
static void colm_reference(const HostArgs& a, int u, Unit* out, int* t) {
  const int st = a.g[0].steps;
  const int per = a.ntm * st;
  const int nt = u / per;
  const int r2 = u - nt * per;
  const int mt = r2 / st;
  *t = nt * a.ntm + mt;
  const int nt2 = *t / a.ntm;                     // its tile_of
  *out = Unit{0, *t - nt2 * a.ntm, nt2, r2 - mt * st};
}

// 1 (second half) and 8: every unit's (tile, stage) as locate / tile_of name it against the nested-loop reference
template <int ORDER>
static void check_locate(const HostArgs& a, const std::vector<Unit>& ref, bool strip) {
  for (int u = 0; u < (int)ref.size(); ++u) {
    int t, k, steps;
    locate<ORDER>(a, u, &t, &k, &steps);
    Piece p{};
    tile_of<ORDER>(a, t, &p);
    const Unit& r = ref[u];
    if (p.gi != r.gi || p.mt != r.mt || p.nt != r.nt || k != r.k || steps != a.g[r.gi].steps) fail("locate / tile_of against the nested loops", u, t);
    if (!strip && a.ngroups == 1) {
      Unit c;
      int tc;
      colm_reference(a, u, &c, &tc);
      if (tc != t || c.gi != p.gi || c.mt != p.mt || c.nt != p.nt || c.k != k) fail("general column-major rule against the COLM formula", u, t);
    }
  }
}

struct Emitted { Piece p; int tile; };

template <int ORDER>
static void check_walk(const HostArgs& a, const std::vector<Unit>& ref, const std::vector<int>& ustart, bool guaranteed) {
  ++g_walks;
  const int W = a.nworkers;
  std::vector<std::vector<Emitted>> of(W);          // by slot
  std::vector<int> slot_seen(W, 0);
  for (int w = 0; w < W; ++w) {
    PieceWalk<ORDER> walk;
    walk.init(a, w);
    const int wl = walk.wl;
    if (wl != worker_slot(a, w) || wl < 0 || wl >= W || slot_seen[wl]++) { fail("worker slots are no permutation", w, wl); return; }
    Piece p;
    int n = 0;
    while (walk.next(a, &p)) {
      if (++n > (int)ref.size() + 8) { fail("the walk does not end", w); return; }
      if (p.gi < 0 || p.gi >= a.ngroups || p.mt < 0 || p.mt >= a.ntm || p.nt < 0 || p.nt >= a.g[p.gi].ntn || p.k0 < 0 || p.k0 >= p.k1 ||
          p.k1 > a.g[p.gi].steps) {
        fail("piece outside the launch", w, n);
        return;
      }
      of[wl].push_back(Emitted{p, tile_index(a, p.gi, p.mt, p.nt)});
    }
    if (walk.next(a, &p)) fail("a finished walk starts again", w);
    const int u_lo = share_begin(a, wl), u_hi = share_begin(a, wl + 1);
    if (u_hi <= u_lo && n != 0) fail("5: a worker with an empty share emitted a piece", w, n);      // 5
    g_pieces += n;
  }
  if (!guaranteed) return;                          // shares shorter than a tile: only 5 is promised
  std::vector<int> covered(ref.size(), 0), first_worker(ustart.size(), -1), workers_on(ustart.size(), 0);
  for (int wl = 0; wl < W; ++wl) {
    const int u_lo = share_begin(a, wl), u_hi = share_begin(a, wl + 1);
    int pub = -1, con = -1;
    for (int i = 0; i < (int)of[wl].size(); ++i) {
      const Piece& p = of[wl][i].p;
      const int tile = of[wl][i].tile;
      for (int k = p.k0; k < p.k1; ++k) {            // 1: inside the share, each unit once
        const int u = ustart[tile] + k;
        if (u < u_lo || u >= u_hi) fail("1: a piece leaves its worker's share", wl, u);
        ++covered[u];
      }
      if (first_worker[tile] != wl) { first_worker[tile] = wl; ++workers_on[tile]; }      // (slots are visited in turn)
      if (p.split != 0) fail("stream-K piece with a split index", wl);
      if (p.publish) {
        if (pub >= 0) fail("4: two publishing pieces", wl);
        pub = i;
        if (p.k0 != 0 || p.k1 >= a.g[p.gi].steps || p.consume >= 0) fail("a head is the first stages of a tile, from zero", wl);
        int partners = 0;                            // 2
        if (wl + 1 < W)
          for (const Emitted& q : of[wl + 1])
            if (q.tile == tile && q.p.consume == wl && q.p.k0 == p.k1) ++partners;
        if (partners != 1) fail("2: a published piece needs exactly one partner", wl, partners);
      }
      if (p.consume >= 0) {
        if (con >= 0) fail("4: two consuming pieces", wl);
        con = i;
        if (wl == 0) fail("3: worker 0 consumes", wl);
        if (p.consume != wl - 1 || p.k0 == 0 || p.k1 != a.g[p.gi].steps) fail("a tail continues worker w - 1 to the tile's end", wl, p.consume);
        int publishers = 0;
        if (wl > 0)
          for (const Emitted& q : of[wl - 1])
            if (q.tile == tile && q.p.publish && q.p.k1 == p.k0) ++publishers;
        if (publishers != 1) fail("2: a consuming piece needs exactly one publisher", wl, publishers);
      }
      if (!p.publish && p.consume < 0 && (p.k0 != 0 || p.k1 != a.g[p.gi].steps)) fail("a piece that is neither head nor tail is a whole tile", wl);
    }
    if (pub >= 0 && con >= 0) {                      // 4
      if (con < pub) fail("4: a worker consumes before it has published", wl);
      if (of[wl][pub].tile == of[wl][con].tile) fail("4: head and tail are the same tile", wl);
    }
    if (pub > 0) fail("4: the head is not the worker's first piece", wl, pub);
  }
  for (size_t u = 0; u < covered.size(); ++u)
    if (covered[u] != 1) { fail("1: a unit is not covered exactly once", (int)u, covered[u]); break; }
  for (size_t t = 0; t < workers_on.size(); ++t)
    if (workers_on[t] > 2) { fail("2: a tile is touched by more than two workers", (int)t, workers_on[t]); break; }
}

static void check_stream_k(HostArgs a) {
  a.sk = 1;
  a.ksplit = 1;
  fill(a);
  int max_steps = 0;
  for (int gi = 0; gi < a.ngroups; ++gi) max_steps = std::max(max_steps, a.g[gi].steps);
  const int bound = (int)(a.units / max_steps) & ~7;        // the host's guarantee: a share is at least a longest tile (schedule)
  if (bound < 8) return;
  ++g_geometries;
  for (int order : {kOrderStrip, kOrderColumn}) {
    a.order = order;
    g_order_now = order;
    g_now = &a;
    const bool strip = order == kOrderStrip;
    const std::vector<Unit> ref = reference_units(a, strip);
    if ((long long)ref.size() != a.units) { fail("unit count"); return; }
    std::vector<int> ustart((size_t)a.tps * a.ntm, -1);
    for (int u = 0; u < (int)ref.size(); ++u)
      if (ref[u].k == 0) ustart[tile_index(a, ref[u].gi, ref[u].mt, ref[u].nt)] = u;
    check_locate<kOrderRuntime>(a, ref, strip);
    if (strip) check_locate<kOrderStrip>(a, ref, strip);
    else if (a.ngroups == 1) check_locate<kOrderColumn>(a, ref, strip);      // the compile-time form skips the group search
    for (a.nworkers = 8; a.nworkers <= bound; a.nworkers += 8) {
      check_walk<kOrderRuntime>(a, ref, ustart, true);        // bf3_kernel's instantiation
      if (strip) check_walk<kOrderStrip>(a, ref, ustart, true);        // gg_kernel's
      else if (a.ngroups == 1) check_walk<kOrderColumn>(a, ref, ustart, true);      // its COLM twin's: single-group launches only
    }
  }
}

static void check_static(HostArgs a) {
  for (int ksplit : {1, 2, 3, 5}) {
    a.sk = 0;
    a.ksplit = ksplit;
    a.nworkers = 0;
    a.order = kOrderStrip;
    fill(a);
    g_now = &a;
    g_order_now = a.order;
    ++g_geometries;
    const int tiles = a.tps * a.ntm;
    {
      PieceWalk<kOrderStrip> walk;                   // a static launch is its one piece: the walk has nothing to add
      Piece q;
      if (walk.next(a, &q)) fail("a static launch's walk yields a piece");
    }
    std::vector<int> k0(tiles * ksplit, -1), k1(tiles * ksplit, -1);
    for (int b = 0; b < tiles * ksplit; ++b) {
      Piece p;
      static_piece(a, b, &p);
      ++g_pieces;
      if (p.gi < 0 || p.gi >= a.ngroups || p.mt < 0 || p.mt >= a.ntm || p.nt < 0 || p.nt >= a.g[p.gi].ntn || p.split < 0 || p.split >= ksplit ||
          p.consume != -1 || p.publish != 0) {
        fail("6: static piece outside the launch", b);
        return;
      }
      const int key = tile_index(a, p.gi, p.mt, p.nt) * ksplit + p.split;
      if (k0[key] != -1) fail("6: two blocks on one (tile, split)", b, key);      // tiles * ksplit blocks, none twice: one-to-one
      k0[key] = p.k0;
      k1[key] = p.k1;
      const int steps = a.g[p.gi].steps;
      if (p.k0 != (int)((long long)p.split * steps / ksplit) || p.k1 != (int)((long long)(p.split + 1) * steps / ksplit))
        fail("7: K range of a split", b, p.split);
    }
    for (int gi = 0; gi < a.ngroups; ++gi)             // 7: [0, steps) in ksplit consecutive ranges
      for (int mt = 0; mt < a.ntm; ++mt)
        for (int nt = 0; nt < a.g[gi].ntn; ++nt) {
          const int t = tile_index(a, gi, mt, nt) * ksplit;
          bool ok = k0[t] == 0 && k1[t + ksplit - 1] == a.g[gi].steps;
          for (int s = 0; s + 1 < ksplit; ++s) ok = ok && k1[t + s] == k0[t + s + 1] && k0[t + s] <= k1[t + s];
          if (!ok) fail("7: the K ranges of a tile do not partition [0, steps)", gi, mt * 100 + nt);
        }
  }
}

int main() {
  const int step_sets[][kPieceGroups] = {{7, 7, 7, 7},          // equal
                                         {18, 12, 12, 8},       // the 5x5 / 2 transposed family
                                         {12, 18, 8, 12},
                                         {40, 1, 3, 40}};       // one long and one very short group
  const int ntn_sets[][kPieceGroups] = {{1, 1, 1, 1}, {5, 5, 5, 5}, {1, 2, 3, 4}, {5, 3, 1, 2}, {2, 5, 4, 1}, {3, 1, 5, 3}, {4, 4, 2, 5}};
  for (int ngroups = 1; ngroups <= kPieceGroups; ++ngroups)
    for (auto& steps : step_sets)
      for (auto& ntn : ntn_sets)
        for (int ntm : {1, 7, 8, 9, 16, 19}) {
          HostArgs a{};
          a.ngroups = ngroups;
          a.ntm = ntm;
          for (int gi = 0; gi < ngroups; ++gi) { a.g[gi].steps = steps[gi]; a.g[gi].ntn = ntn[gi]; }
          check_stream_k(a);
          check_static(a);
        }
  {   // 5 alone: more workers than units (outside the host's guarantee, so nothing else is promised)
    HostArgs a{};
    a.sk = 1; a.ngroups = 1; a.ntm = 1; a.ksplit = 1; a.order = kOrderStrip;
    a.g[0].steps = 3; a.g[0].ntn = 1;
    fill(a);
    g_now = &a;
    for (a.nworkers = 8; a.nworkers <= 24; a.nworkers += 8) check_walk<kOrderRuntime>(a, {}, {}, false);
  }
  std::printf("walked %lld geometries (%lld stream-K walks, %lld pieces), %lld mismatches\n", g_geometries, g_walks, g_pieces, g_failed);
  return g_failed == 0 && g_geometries > 0 ? 0 : 1;
}
