// gg_pieces.h -- which stages of which tile a workgroup of a gather GEMM computes, and the stream-K hand-off between two of them:
// the one copy for gg_kernel (gather_gemm_kernel.h, fp32) and bf3_kernel (bf3_gemm.hip, pre-split bf16 x 3).  DESIGN.md 4.1, 4.1b.
//   Part A  the piece walk: plain functions over the launch's tile / unit counts, compiled by the device compiler into the kernels
//           and by any host compiler into tests/gg_pieces_host.cc, which walks every worker of small launches and checks that the
//           pieces cover every (tile, stage) once and that no worker can wait for a hand-off that is never published.
//           `a` is anything with the fields of GGArgs the walk reads (sk, ngroups, ntm, tps, ups, units, nworkers, ksplit, order,
//           g[i].{steps, tile0, unit0, ntn, blk0}): the kernels pass their kernarg view, the host program a plain struct.
//   Part B  device only: the kernarg view, the row table of a piece, and the two sides of the hand-off.
// The host computes its half (tile0, unit0, tps, ups, units) in one place too: work_of, conv_plan.hip.
#pragma once

#if defined(__HIPCC__)
#include "sntc_internal.h"
#define SNTC_PIECE_FN __host__ __device__ __forceinline__
#define SNTC_PIECE_UNROLL _Pragma("unroll")
#else
#define SNTC_PIECE_FN inline
#define SNTC_PIECE_UNROLL
#endif

namespace sntc {

// ------------------------------------------------------------------------------------------------------
// Part A: the piece walk
// ------------------------------------------------------------------------------------------------------
constexpr int kPieceGroups = 4;     // = kMaxGroups (sntc_internal.h)

// One unit of a workgroup's work: stages [k0, k1) of tile (gi, mt, nt).
struct Piece {
  int gi, mt, nt, k0, k1;
  int consume;   // worker whose published accumulators this piece continues (-1: start from zero)
  int publish;   // 1: the tile is finished by the next worker: leave raw accumulators in sk_slab[self]
  int split;     // static split-K: index of this K range (bf3_kernel has no split-K and ignores it)
};

// Stream-K unit order.  Strip-major: row strip, then group, then column tile (u = mt * ups + unit0(g) + nt * steps + k, tile id
// = mt * tps + tile0(g) + nt) -- every worker's share mixes the groups (their tiles differ in length, so a group-major order
// would hand some workers only short, epilogue-heavy tiles) and one strip's input rows serve all groups while they are hot in L2.
// Column-major: COLUMN tile outermost, row strips inside (u = ntm * unit0(g) + nt * ntm * steps + mt * steps + k, tile id =
// (tile0(g) + nt) * ntm + mt).  The workers of one XCD own a contiguous eighth of the range, i.e. less than one column tile of a
// five-column layer, whose weight rows then stay in that XCD's 4 MB L2 while the strips stream past -- for layers whose packed
// weights exceed the L2 (hyper-synthesis 480 -> 640: 11 MB), where the strip-major order streams the whole matrix through every
// XCD once per strip.  gg_kernel takes the order at compile time (the COLM twin, single-group plans: round 3 had it as a run-time
// branch and the branch moved the whole kernel's register allocation); bf3_kernel reads GGArgs::order (its A/B switch: measured
// equal on single-group layers and 20 % slower on the four-group synthesis).  The column-major rule is one formula for any
// number of groups; the compile-time form is launched with one group only (column_major, conv_plan.hip) and skips the group
// search: with the search the twin needs 169 instead of 168 VGPRs and loses its third wave per SIMD.
enum { kOrderRuntime = -1, kOrderColumn = 0, kOrderStrip = 1 };   // >= 0: the values of GGArgs::order
template <int ORDER, class A>
SNTC_PIECE_FN bool strip_major(const A& a) { return ORDER == kOrderRuntime ? a.order == kOrderStrip : ORDER == kOrderStrip; }

// the last group i whose first tile / unit / block is reached (`reached(i)`), 0 if none
template <class A, class F>
SNTC_PIECE_FN int group_at(const A& a, F&& reached) {
  int gi = 0;
  SNTC_PIECE_UNROLL
  for (int i = 1; i < kPieceGroups; ++i)
    if (i < a.ngroups && reached(i)) gi = i;
  return gi;
}

// Worker (workgroup) w -> its slot in the unit range: the workers on one XCD (w, w + 8, ...) own one contiguous eighth.  Slot wl
// owns the units [share_begin(wl), share_begin(wl + 1)), publishes into sk_slab[wl] and continues the chain of slot wl - 1.
template <class A>
SNTC_PIECE_FN int worker_slot(const A& a, int w) { return (w & 7) * (a.nworkers >> 3) + (w >> 3); }
template <class A>
SNTC_PIECE_FN int share_begin(const A& a, int wl) { return (int)(a.units * wl / a.nworkers); }

// unit u -> (global tile id, stage inside the tile, stages of the tile)
template <int ORDER, class A>
SNTC_PIECE_FN void locate(const A& a, int u, int* t, int* k, int* steps) {
  int gi;
  if (strip_major<ORDER>(a)) {
    const int mt = u / a.ups;
    const int r = u - mt * a.ups;
    gi = group_at(a, [&](int i) { return r >= (int)a.g[i].unit0; });
    const int r2 = r - (int)a.g[gi].unit0;
    const int nt = r2 / a.g[gi].steps;
    *t = mt * a.tps + a.g[gi].tile0 + nt;
    *k = r2 - nt * a.g[gi].steps;
  } else {
    gi = ORDER == kOrderColumn ? 0 : group_at(a, [&](int i) { return u >= (int)a.g[i].unit0 * a.ntm; });
    const int r = u - (int)a.g[gi].unit0 * a.ntm;
    const int per = a.ntm * a.g[gi].steps;
    const int nt = r / per;
    const int r2 = r - nt * per;
    const int mt = r2 / a.g[gi].steps;
    *t = (a.g[gi].tile0 + nt) * a.ntm + mt;
    *k = r2 - mt * a.g[gi].steps;
  }
  *steps = a.g[gi].steps;
}

// global tile id -> (group, row strip, column tile)
template <int ORDER, class A>
SNTC_PIECE_FN void tile_of(const A& a, int t, Piece* p) {
  const bool strip = strip_major<ORDER>(a);
  const int mt = strip ? t / a.tps : t % a.ntm;
  const int r = strip ? t - mt * a.tps : t / a.ntm;
  const int gi = ORDER == kOrderColumn ? 0 : group_at(a, [&](int i) { return r >= a.g[i].tile0; });
  p->gi = gi; p->mt = mt; p->nt = r - a.g[gi].tile0;
}

// A stream-K worker's list of pieces: [head piece of the LAST tile of its share (published)] [whole tiles] [tail piece of the
// FIRST tile].  The head depends on nothing and goes first; the tail continues the previous worker's chain, whose head was
// computed first thing, so the tail never waits.  Whole-tiles-first was tried for lockstep L2 sharing: the tails then wait for
// heads of uneven length and the remainder phase doubles (HS2 172 -> 124 TFLOP/s-equivalent).
// Host guarantee (schedule, conv_plan.hip): a share is at least as long as the longest tile, so head and tail are different tiles
// and a tile is cut between at most two workers.
template <int ORDER>
struct PieceWalk {
  int head_t = -1, head_k1 = 0;     // global tile id / end stage of the head piece
  int tail_t = -1, tail_k0 = 0;     // ... / start stage of the tail piece
  int cur = 0, last = -1;           // whole tiles [cur, last]
  int phase = 0;                    // 0 head, 1 whole tiles, 2 tail, 3 done
  int wl = 0;

  template <class A>
  SNTC_PIECE_FN void init(const A& a, int w) {
    wl = worker_slot(a, w);
    const int u_lo = share_begin(a, wl), u_hi = share_begin(a, wl + 1);
    if (u_hi <= u_lo) { phase = 3; return; }
    int tF, kF, sF, tL, kL, sL;
    locate<ORDER>(a, u_lo, &tF, &kF, &sF);
    locate<ORDER>(a, u_hi - 1, &tL, &kL, &sL);
    cur = tF;
    last = tL;
    if (kF > 0) { tail_t = tF; tail_k0 = kF; cur = tF + 1; }
    if (kL + 1 < sL) { head_t = tL; head_k1 = kL + 1; last = tL - 1; }
  }

  template <class A>
  SNTC_PIECE_FN bool next(const A& a, Piece* p) {
    if (!a.sk) return false;          // a static launch is its one piece
    p->k0 = 0; p->consume = -1; p->publish = 0; p->split = 0;
    if (phase == 0) {
      phase = 1;
      if (head_t >= 0) {
        tile_of<ORDER>(a, head_t, p);
        p->k1 = head_k1; p->publish = 1;
        return true;
      }
    }
    if (phase == 1) {
      if (cur <= last) {
        tile_of<ORDER>(a, cur++, p);
        p->k1 = a.g[p->gi].steps;
        return true;
      }
      phase = 2;
    }
    if (phase == 2) {
      phase = 3;
      if (tail_t >= 0) {
        tile_of<ORDER>(a, tail_t, p);
        p->k0 = tail_k0; p->k1 = a.g[p->gi].steps; p->consume = wl - 1;
        return true;
      }
    }
    return false;
  }
};

// Static mode: one workgroup per (tile, K range); block `b` of the launch -> its piece.  K ranges > 1 leave raw partial sums for
// gg_reduce_kernel (deterministic split-K); pre-split launches always have ksplit == 1 (schedule_s3).
template <class A>
SNTC_PIECE_FN void static_piece(const A& a, int b, Piece* p) {
  const int gi = group_at(a, [&](int i) { return b >= a.g[i].blk0; });
  const int lb0 = b - a.g[gi].blk0;
  const int split = lb0 % a.ksplit;
  const int lb = lb0 / a.ksplit;
  // XCD-aware tile order: blocks b and b + 8 share an XCD (and its 4 MB L2).  Inside one XCD's sequence the column
  // tile runs fastest, so the blocks resident on an XCD cover a few row strips x all column tiles.
  const int ntn = a.g[gi].ntn;
  const int full = a.ntm & ~7;
  if (lb < full * ntn) {
    const int l = lb >> 3;
    p->mt = (l / ntn) * 8 + (lb & 7);
    p->nt = l % ntn;
  } else {                                   // ragged tail: fewer than 8 row strips left
    const int r = lb - full * ntn, rem = a.ntm - full;
    p->mt = full + r % rem;
    p->nt = r / rem;
  }
  const int steps = a.g[gi].steps;
  p->gi = gi;
  p->k0 = (int)(((long long)split * steps) / a.ksplit);
  p->k1 = (int)(((long long)(split + 1) * steps) / a.ksplit);
  p->consume = -1; p->publish = 0; p->split = split;
}

#if defined(__HIPCC__)
// ------------------------------------------------------------------------------------------------------
// Part B: device side
// ------------------------------------------------------------------------------------------------------
static_assert(kPieceGroups == kMaxGroups, "the walk's group loops cover GGArgs::g");

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

constexpr unsigned kOutOfRange = 0x80000000u;   // > any in-range offset: buffers are < 2 GiB (host check)
constexpr int kSpinLimit = 1 << 22;             // bounded wait on a neighbour's hand-off (~seconds), then the launch is flagged invalid

__device__ __forceinline__ float apply_act(float v, int act) {
  switch (act) {
    case SNTC_ACT_RELU: return fmaxf(v, 0.0f);
    case SNTC_ACT_LEAKY_RELU: return v >= 0.0f ? v : 0.2f * v;
    case SNTC_ACT_SIGMOID: return 1.0f / (1.0f + expf(-v));
    default: return v;
  }
}

// The kernel arguments through an OPAQUE pointer to the kernarg segment: loads through it cannot be hoisted out of the
// persistent tile loop, so a phase that runs once per tile (piece bookkeeping, row table, epilogue) re-reads its few
// scalars from the scalar cache instead of pinning ~60 SGPRs (and, once those run out, VGPRs) through the K loop.
typedef const GGArgs __attribute__((address_space(4))) KArgs;
__device__ __forceinline__ KArgs& fresh_args() {
  KArgs* kp = (KArgs*)__builtin_amdgcn_kernarg_segment_ptr();
  asm volatile("" : "+s"(kp));
  return *kp;
}

// (n, qy, qx, valid) of the BM rows of piece `p` into `rinfo`, by NT threads; the caller synchronises before reading it
template <int BM, int NT>
__device__ __forceinline__ void write_rinfo(KArgs& a, const Piece& p, int4* rinfo, int tid) {
  const int mbase = p.mt * BM;
  const int q0y = a.g[p.gi].q0y, q0x = a.g[p.gi].q0x;
  for (int r = tid; r < BM; r += NT) {
    const int m = mbase + r;
    int4 ri = make_int4(0, 0, 0, 0);
    if (m < a.M) {
      const int per = a.Qh * a.Qw;
      const int n = m / per;
      const int rem = m - n * per;
      const int qy = rem / a.Qw;
      ri = make_int4(n, qy + q0y, rem - qy * a.Qw + q0x, 1);   // per-group origin of the macro grid
    }
    rinfo[r] = ri;
  }
}

// A worker's hand-off slab: [TM * TN * 4 quads][NT threads][4 floats], raw accumulators in register layout: 16 B per lane, 1 KB
// per wave instruction, NT * 16 B per quad; addressed through a buffer descriptor with constant scalar offsets (no per-access
// 64-bit address registers)
template <int TM, int TN, int NT>
__device__ __forceinline__ __amdgpu_buffer_rsrc_t sk_slab_of(float* sk_slab, int worker) {
  return __builtin_amdgcn_make_buffer_rsrc(sk_slab + (size_t)worker * (TM * TN * 16 * NT), 0, TM * TN * 16 * NT * 4, 0x00020000);
}

// Stream-K hand-off, consumer side: the accumulators start from what `worker` published.
template <int TM, int TN, int NT, class A>
__device__ __forceinline__ void sk_consume(const A& a, int worker, int tid, f32x16 (&acc)[TM][TN]) {
  if (tid == 0) {
    int spins = 0;
    while (__hip_atomic_load(a.sk_flags + worker, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0) {
      __builtin_amdgcn_s_sleep(8);
      if (++spins > kSpinLimit) {
        // a neighbour that never published (it cannot be co-resident: HIP promises neither residency nor dispatch
        // order): never hang and never take the context down -- flag the launch as invalid and carry on with whatever
        // the slab holds; the host reads the sticky word at its next synchronisation point (sntc_conv_status), raises,
        // and can re-run on the static schedule (sntc_conv_set_stream_k(0))
        __hip_atomic_fetch_or(fresh_args().status, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        break;
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  }
  __syncthreads();
  const __amdgpu_buffer_rsrc_t sr = sk_slab_of<TM, TN, NT>(a.sk_slab, worker);
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(sr, tid * 16, ((i * TN + j) * 4 + q) * NT * 16, 0);
        const f32x4 f = __builtin_bit_cast(f32x4, v);
        acc[i][j][4 * q] = f[0]; acc[i][j][4 * q + 1] = f[1]; acc[i][j][4 * q + 2] = f[2]; acc[i][j][4 * q + 3] = f[3];
      }
}

// Producer side (cdna_hip_programming.md Guideline 16): plain stores, every wave drains its stores, workgroup barrier, ONE
// agent-scope release, then the flag.
template <int TM, int TN, int NT, class A>
__device__ __forceinline__ void sk_publish(const A& a, int wl, int tid, const f32x16 (&acc)[TM][TN]) {
  const __amdgpu_buffer_rsrc_t sr = sk_slab_of<TM, TN, NT>(a.sk_slab, wl);
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const f32x4 v = {acc[i][j][4 * q], acc[i][j][4 * q + 1], acc[i][j][4 * q + 2], acc[i][j][4 * q + 3]};
        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), sr, tid * 16, ((i * TN + j) * 4 + q) * NT * 16, 0);
      }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (tid == 0) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __hip_atomic_store(a.sk_flags + wl, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}
#endif   // __HIPCC__

}  // namespace sntc
