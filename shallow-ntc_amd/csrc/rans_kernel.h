// rans_kernel.h -- the rANS coder's device code, once: one encoder body and one decoder body (stream format: the head of
// rans.hip), templated on where a lane's (table id, value) comes from and where the value goes:
//   IdEnc / IdDec (rans.hip)                table ids from a uint16 tensor through a chunk-ahead LDS ring, int32 values;
//   ChannelEnc / ChannelDec (rans_channels.hip)   table = channel = e % C of the flat NHWC index, carried by the lane (+= L % C with a
//                                           wrap: no id tensor, no id ring), floats in (rounded when they reach the ring), floats out;
// and, for the decoder, on how a slot finds its symbol: CdfSearch (binary search of RansTables, in LDS or in global memory) or
// StartTableSearch (RansDecTables in LDS).  A source is plain per-lane state with forced-inline members: nothing of it survives
// compilation but the registers it names.  The __global__ kernels of the two files are instantiations; their host launchers
// share rans_launch() and rans_dec_tables() below.
#pragma once
#include <algorithm>
#include <string>
#include <type_traits>
#include "rans_common.h"

namespace sntc {

// staging rings ahead of the tables in dynamic LDS.  Id source: id ring [2][kChunk * 64] uint16, then the encoder's value ring
// [2][kChunk * 64] int or the decoder's word ring [kWordRing] uint16.  Channel source: the value / word ring alone.
constexpr int kIdRingBytes = 2 * kChunk * 64 * 2;
constexpr int kChanStagingBytes = 2 * kChunk * 64 * 4;
constexpr int kStagingBytes = kIdRingBytes + kChanStagingBytes;
static_assert(kWordRing * 2 <= kChanStagingBytes, "the decoder's word ring must fit where the encoder's value ring does");

// stream s = (image b, segment sg) codes elements [e0, e0 + n) of its tensor; r0 = the first one's index within its image.
// A segment's elements fit 32 bits (host: cap_words < 2^30).
struct RansStream {
  long long e0, r0;
  int n, steps, nchunks;
};

__device__ __forceinline__ RansStream rans_stream(int s, int segs, int L, long long E, long long Eseg) {
  const int b = s / segs, sg = s - b * segs;
  RansStream st;
  st.r0 = (long long)sg * Eseg;
  const long long r1 = std::min(E, st.r0 + Eseg);
  st.e0 = (long long)b * E + st.r0;
  st.n = r1 > st.r0 ? (int)(r1 - st.r0) : 0;
  st.steps = (st.n + L - 1) / L;                             // L = lanes in use (8 .. 64): short streams flush fewer states
  st.nchunks = (st.steps + kChunk - 1) / kChunk;
  return st;
}

// ---- element sources, encoder side: fetch(k) loads chunk k into registers (k < 0: nothing), spill(k) drops them into ring
// buffer k & 1, chunk(k) + read(i, t, v) hand out step i of chunk k (i < 0: no step).  The kernel sets the first line of members.
struct IdEnc {
  static constexpr int kStaging = kStagingBytes;
  const int* values;
  const unsigned short* tid;
  unsigned short* tring;
  int* vring;
  const unsigned short* tb;
  const int* vb;
  int nl, L, lane;
  unsigned short TR[kChunk];
  int VR[kChunk];
  __device__ __forceinline__ void init(const RansStream& st, int L_, int lane_, unsigned char* smem) {
    tring = reinterpret_cast<unsigned short*>(smem);
    vring = reinterpret_cast<int*>(smem + kIdRingBytes);
    values += st.e0;
    tid += st.e0;
    L = L_;
    lane = lane_;
    nl = lane < L ? st.n : 0;                                // the lane has an element at position r of the stream iff r < nl
  }
  __device__ __forceinline__ void fetch(int k) {
#pragma unroll
    for (int i = 0; i < kChunk; ++i) {
      const int r = (k * kChunk + i) * L + lane;
      const bool a = k >= 0 && r < nl;
      TR[i] = a ? tid[r] : kNoTable;
      VR[i] = a ? values[r] : 0;
    }
  }
  __device__ __forceinline__ void spill(int k) {
#pragma unroll
    for (int i = 0; i < kChunk; ++i) {
      tring[(k & 1) * kChunk * 64 + i * 64 + lane] = TR[i];
      vring[(k & 1) * kChunk * 64 + i * 64 + lane] = VR[i];
    }
  }
  __device__ __forceinline__ void chunk(int k) {
    tb = tring + (k & 1) * kChunk * 64 + lane;
    vb = vring + (k & 1) * kChunk * 64 + lane;
  }
  __device__ __forceinline__ void read(int i, int& t, int& v) {
    const int ii = std::max(i, 0);
    t = tb[ii * 64];
    v = vb[ii * 64];
    if (i < 0) t = kNoTable;
  }
};

// the floats stay in registers, untouched, while the chunk before them is coded (their loads are in flight meanwhile); they are
// rounded (rintf: half to even, what round_to_int_kernel and the prior scan's y_hat do), and written back as y_hat where that is
// asked for, when they are dropped into the ring.  The steps are read in strictly descending order (last step of the last chunk
// first), so the lane carries the position rq and the table id tq of the next step to read: -L and -(L % C) with a wrap per step.
struct ChannelEnc {
  static constexpr int kStaging = kChanStagingBytes;
  const float* y;
  float* y_hat;
  int C;
  long long e0;
  int* vring;
  const int* vb;
  int nl, L, lane, lstep, rq, tq;
  float FR[kChunk];
  __device__ __forceinline__ void init(const RansStream& st, int L_, int lane_, unsigned char* smem) {
    vring = reinterpret_cast<int*>(smem);
    e0 = st.e0;
    L = L_;
    lane = lane_;
    nl = lane < L ? st.n : 0;
    lstep = L % C;
    rq = (st.steps - 1) * L + lane;
    tq = st.steps > 0 ? (int)((st.r0 % C + rq) % C) : 0;     // E % C == 0: an image's first element is channel 0
  }
  // k < 0 is tested once, not per element: as part of each element's condition the compiler moves the rounding up to the load
  __device__ __forceinline__ void fetch(int k) {
    if (k < 0) {
#pragma unroll
      for (int i = 0; i < kChunk; ++i) FR[i] = 0.0f;
      return;
    }
#pragma unroll
    for (int i = 0; i < kChunk; ++i) {
      const int r = (k * kChunk + i) * L + lane;
      FR[i] = r < nl ? y[e0 + r] : 0.0f;
    }
  }
  __device__ __forceinline__ void spill(int k) {
#pragma unroll
    for (int i = 0; i < kChunk; ++i) {
      const int v = (int)rintf(FR[i]);
      vring[(k & 1) * kChunk * 64 + i * 64 + lane] = v;
      const int r = (k * kChunk + i) * L + lane;
      if (y_hat && k >= 0 && r < nl) y_hat[e0 + r] = (float)v;
    }
  }
  __device__ __forceinline__ void chunk(int k) { vb = vring + (k & 1) * kChunk * 64 + lane; }
  __device__ __forceinline__ void read(int i, int& t, int& v) {
    if (i < 0) {
      t = kNoTable;
      v = 0;
      return;
    }
    t = rq < nl ? tq : (int)kNoTable;
    v = vb[i * 64];
    rq -= L;
    tq -= lstep;
    tq += tq < 0 ? C : 0;
  }
};

// One wave per stream.  Everything that depends only on the symbol (descriptor, ESCAPE test, f, c) runs two steps ahead of the
// state arithmetic; the loop-carried chain is: escape emit, renormalise, divide.
template <bool LDS, class Src>
__device__ __forceinline__ void rans_encode_body(Src& src, int segs, int L, long long E, long long Eseg, const RansTables& T,
                                                 long long cap, unsigned short* __restrict__ scratch, int* __restrict__ len_words) {
  extern __shared__ unsigned char smem[];
  const uint2* meta;
  const unsigned short* cdf;
  rans_stage_tables<LDS>(T, smem + Src::kStaging, meta, cdf);
  const int s = blockIdx.x, lane = threadIdx.x;
  const RansStream st = rans_stream(s, segs, L, E, Eseg);
  src.init(st, L, lane, smem);
  unsigned short* out = scratch + (size_t)s * cap;
  long long wp = cap;
  const unsigned long long gt = lane == 63 ? 0ull : (~0ull << (lane + 1));
  unsigned x = 1u << 16;

  struct Sym { unsigned f, c, raw; bool active, esc; };
  auto lookup = [&](int t, int v, uint2 m) -> Sym {
    const bool active = t != kNoTable;
    const int n = (int)(m.y >> 16);
    bool esc;
    int sym = rans_symbol(v, m, esc);
    esc = active && esc;
    if (!active) sym = 0;
    const unsigned at = m.x + sym, last = m.x + n - 1;       // the symbol's cdf entry and the table's last one: one address sum
    const unsigned cl = cdf[at];
    const unsigned ch = at < last ? (unsigned)cdf[at + 1] : 65536u;
    return Sym{active ? ch - cl : 1u, cl, (unsigned)(std::min(std::max(v, -32768), 32767) + 32768), active, esc};
  };
  if (st.nchunks > 0) {
    src.fetch(st.nchunks - 1);
    src.spill(st.nchunks - 1);
  }
  for (int k = st.nchunks - 1; k >= 0; --k) {
    src.fetch(k - 1);
    src.chunk(k);
    const int cnt = std::min(kChunk, st.steps - k * kChunk);
    int t1, v1, t2, v2;
    src.read(cnt - 1, t1, v1);
    Sym cur = lookup(t1, v1, meta[t1 == kNoTable ? 0 : t1]);
    src.read(cnt - 2, t1, v1);
    uint2 m1 = meta[t1 == kNoTable ? 0 : t1];
    src.read(cnt - 3, t2, v2);
    for (int i = cnt - 1; i >= 0; --i) {
      const Sym sy = cur;
      cur = lookup(t1, v1, m1);                             // step i - 1
      t1 = t2;
      v1 = v2;
      m1 = meta[t1 == kNoTable ? 0 : t1];                   // step i - 2
      src.read(i - 3, t2, v2);
      const unsigned long long emask = __ballot(sy.esc);
      if (emask) {                                          // value first (reverse order), then the ESCAPE symbol
        if (sy.esc) {
          out[wp - 1 - __popcll(emask & gt)] = (unsigned short)(x & 0xffffu);
          x = (x & 0xffff0000u) | sy.raw;
        }
        wp -= __popcll(emask);
      }
      const bool need = sy.active && (unsigned long long)x >= ((unsigned long long)sy.f << 16);
      const unsigned long long mask = __ballot(need);
      if (need) {
        out[wp - 1 - __popcll(mask & gt)] = (unsigned short)(x & 0xffffu);
        x >>= 16;
      }
      wp -= __popcll(mask);
      if (sy.active) x = ((x / sy.f) << 16) + (x % sy.f) + sy.c;
    }
    src.spill(k - 1);
  }
  wp -= 2 * L;
  if (lane < L) {
    out[wp + 2 * lane] = (unsigned short)(x >> 16);
    out[wp + 2 * lane + 1] = (unsigned short)(x & 0xffffu);
  }
  if (lane == 0) len_words[s] = (int)(cap - wp);
}

// The decoder's stream words: the ring holds [ptr, ptr + kWordRing) at the start of a chunk; a chunk eats at most kWordRing / 2.
// ptr = the wave's shared read pointer.  Stream positions fit 32 bits (a longer stream is refused before this is built).
struct WordRing {
  const unsigned short* w;
  unsigned short* ring;
  int len, lane, ptr, filled, wfrom, wto;
  unsigned short WR[kWordRegs];
  __device__ __forceinline__ void fetch(int target) {
    wfrom = filled;
    wto = std::min(target, len);
#pragma unroll
    for (int i = 0; i < kWordRegs; ++i) {
      const int q = wfrom + i * 64 + lane;
      WR[i] = q < wto ? w[q] : (unsigned short)0;
    }
  }
  __device__ __forceinline__ void spill() {
#pragma unroll
    for (int i = 0; i < kWordRegs; ++i) {
      const int q = wfrom + i * 64 + lane;
      if (q < wto) ring[q & (kWordRing - 1)] = WR[i];
    }
    filled = std::max(filled, wto);
  }
};

// ---- element sources, decoder side: the table id of a lane's next steps and where its values go.  init() places the source's
// own ring and returns where the word ring goes; fetch(k) / spill(k) stage the ids of chunk k; start() / chunk() load the first
// descriptor of the stream / of a chunk; active() = the lane has an element in the step at hand; advance() moves on to the
// next step's descriptor.  FULL: every lane has an element in every step of the chunk.
struct IdDec {
  static constexpr int kStaging = kStagingBytes;
  using Out = int;
  const unsigned short* tid;
  Out* out;
  unsigned short* tring;
  const unsigned short* tb;
  int nl, L, lane, nchunks, t1, t2;
  unsigned short TR[kChunk];
  __device__ __forceinline__ unsigned short* init(const RansStream& st, int L_, int lane_, unsigned char* smem) {
    tring = reinterpret_cast<unsigned short*>(smem);
    tid += st.e0;
    L = L_;
    lane = lane_;
    nl = lane < L ? st.n : 0;
    nchunks = st.nchunks;
    return tring + 2 * kChunk * 64;
  }
  __device__ __forceinline__ void fetch(int k) {
#pragma unroll
    for (int i = 0; i < kChunk; ++i) {
      const int r = (k * kChunk + i) * L + lane;
      TR[i] = (k < nchunks && r < nl) ? tid[r] : kNoTable;
    }
  }
  __device__ __forceinline__ void spill(int k) {
#pragma unroll
    for (int i = 0; i < kChunk; ++i) tring[(k & 1) * kChunk * 64 + i * 64 + lane] = TR[i];
  }
  template <class D>
  __device__ __forceinline__ void start(const D*, D&) {}
  template <class D>
  __device__ __forceinline__ void chunk(int k, int cnt, const D* desc, D& m1) {
    tb = tring + (k & 1) * kChunk * 64 + lane;
    t1 = tb[0];
    m1 = desc[t1 == kNoTable ? 0 : t1];
    t2 = cnt > 1 ? (int)tb[64] : (int)kNoTable;
  }
  __device__ __forceinline__ bool active() const { return t1 != kNoTable; }
  template <bool FULL, class D>
  __device__ __forceinline__ void advance(int i, int cnt, const D* desc, D& m1) {
    t1 = t2;
    m1 = desc[(!FULL && t1 == kNoTable) ? 0 : t1];           // descriptor of step i + 1
    t2 = tb[std::min(i + 2, kChunk - 1) * 64];               // table id of step i + 2 (FULL: past the chunk a repeat, unused)
    if (!FULL && i + 2 >= cnt) t2 = kNoTable;
  }
};

// the lane's position in the stream and its table id, step by step: +L and +(L % C) with a wrap
struct ChannelDec {
  static constexpr int kStaging = kChanStagingBytes;
  using Out = float;
  Out* out;
  int C;
  int nl, L, lstep, rq, t1;
  __device__ __forceinline__ unsigned short* init(const RansStream& st, int L_, int lane, unsigned char* smem) {
    L = L_;
    nl = lane < L ? st.n : 0;
    lstep = L % C;
    rq = lane;
    t1 = ((int)(st.r0 % C) + lane) % C;                      // E % C == 0: an image's first element is channel 0
    return reinterpret_cast<unsigned short*>(smem);
  }
  __device__ __forceinline__ void fetch(int) {}
  __device__ __forceinline__ void spill(int) {}
  template <class D>
  __device__ __forceinline__ void start(const D* desc, D& m1) { m1 = desc[t1]; }
  template <class D>
  __device__ __forceinline__ void chunk(int, int, const D*, D&) {}
  __device__ __forceinline__ bool active() const { return rq < nl; }
  template <bool FULL, class D>
  __device__ __forceinline__ void advance(int, int, const D* desc, D& m1) {
    rq += L;
    t1 += lstep;
    t1 -= t1 >= C ? C : 0;
    m1 = desc[t1];                                           // descriptor of the next step
  }
};

// ---- symbol searches: stage() puts the tables where the steps read them; step() takes one symbol off the lane's state x,
// refills from the shared pointer (lanes with x < 2^16 each take ONE word, in lane order) and returns the value.

// Binary search of cdf per symbol: tables in LDS, or in global memory where they do not fit.
template <bool LDS>
struct CdfSearch {
  using Tables = RansTables;
  using Desc = uint2;
  const uint2* desc;
  const unsigned short* cdf;
  int qmax;                                                  // the highest stream position the lane took a word from
  __device__ __forceinline__ void stage(const RansTables& T, unsigned char* smem) {
    rans_stage_tables<LDS>(T, smem, desc, cdf);
    qmax = -1;
  }
  __device__ __forceinline__ int step(bool active, uint2 m, unsigned& x, WordRing& R) {
    const unsigned long long lt = (1ull << R.lane) - 1ull;
    const int n = active ? (int)(m.y >> 16) : 1, vmin = (int)(short)(m.y & 0xffffu);
    const unsigned short* c = cdf + m.x;
    const unsigned slot = x & 0xffffu;
    // the largest sym with cdf[sym] <= slot; the bracketing cdf values are carried along so that no read follows the search.
    // (A lone wave is issue-bound: the 4-ary, three-probes-per-level form needs fewer LDS round trips but ~4x the instructions
    // per level and measured slower.)
    int lo = 0, hi = n;
    unsigned clo = 0u, chi = 65536u;
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      const unsigned v = c[mid];
      const bool ge = slot >= v;
      lo = ge ? mid : lo;
      clo = ge ? v : clo;
      hi = ge ? hi : mid;
      chi = ge ? chi : v;
    }
    const unsigned xn = (chi - clo) * (x >> 16) + slot - clo;
    x = active ? xn : x;                                     // a select, not a branch: see StartTableSearch::step
    const bool need = active && x < (1u << 16);
    const unsigned long long mask = __ballot(need);
    if (mask) {                                              // one word each, in lane order, from the shared pointer
      if (need) {
        const int q = R.ptr + __popcll(mask & lt);
        qmax = std::max(qmax, q);
        x = (x << 16) | R.ring[q & (kWordRing - 1)];
      }
      R.ptr += __popcll(mask);
    }
    int v = lo + vmin;
    const bool esc = active && lo == n - 1;
    const unsigned long long emask = __ballot(esc);
    if (emask) {
      if (esc) {
        const int q = R.ptr + __popcll(emask & lt);
        qmax = std::max(qmax, q);
        v = (int)(x & 0xffffu) - 32768;
        x = (x & 0xffff0000u) | R.ring[q & (kWordRing - 1)];
      }
      R.ptr += __popcll(emask);
    }
    return v;
  }
};

// The RansDecTables in LDS.  A lone wave per stream is bound by its chain of dependent LDS round trips and by its own instruction
// issue (nobody to interleave with), so a step is: start symbol from the start table (1 read), four consecutive entries from
// there (independent reads; the symbol is among the first three in > 98 % of the slots of every table, else the round repeats
// from the fourth), refill word (1 read) -- three round trips instead of the binary search's log2(n) + 2 (11 + 2 on the widest
// scale table, and a wave waits for its slowest lane) -- and selects instead of divergent branches.  Decoded values are those of
// CdfSearch, bit for bit (tests/test_hip_bitstream.py).  A word index at or past the stream's end is not checked here: the
// pointer only grows, so it ends past the length and the stream is counted as bad; the ring read itself is masked.
struct StartTableSearch {
  using Tables = RansDecTables;
  using Desc = uint4;                                        // {entry offset, n | vmin, lut offset, 16 - bits}
  const uint4* desc;
  const unsigned* dec;
  const unsigned short* lut;
  static constexpr int qmax = -1;
  __device__ __forceinline__ void stage(const RansDecTables& T, unsigned char* smem) {
    uint4* m4 = reinterpret_cast<uint4*>(smem);
    unsigned* d = reinterpret_cast<unsigned*>(m4 + T.ntables);
    unsigned short* l = reinterpret_cast<unsigned short*>(d + T.dec_total);
    const int lane = threadIdx.x;
    for (int i = lane; i < T.ntables; i += 64) {
      const uint2 a = T.meta[i];
      const unsigned lm = T.lmeta[i];
      m4[i] = make_uint4(a.x + 3u * (unsigned)i, a.y, lm >> 5, 16u - (lm & 31u));
    }
    const uint4* src = reinterpret_cast<const uint4*>(T.dec);
    uint4* dst = reinterpret_cast<uint4*>(d);
    for (int i = lane; i < T.dec_total / 4; i += 64) dst[i] = src[i];
    src = reinterpret_cast<const uint4*>(T.lut);
    dst = reinterpret_cast<uint4*>(l);
    for (int i = lane; i < T.lut_total / 8; i += 64) dst[i] = src[i];
    __syncthreads();
    desc = m4;
    dec = d;
    lut = l;
  }
  __device__ __forceinline__ int step(bool active, uint4 m, unsigned& x, WordRing& R) {
    const unsigned slot = x & 0xffffu, key = (x << 16) | 0xfffeu;
    const unsigned* e = dec + m.x;
    unsigned lo = lut[m.z + (slot >> m.w)];
    unsigned esel;
    for (;;) {
      const unsigned c0 = e[lo], c1 = e[lo + 1], c2 = e[lo + 2], c3 = e[lo + 3];
      asm volatile("" ::"v"(c0), "v"(c1), "v"(c2), "v"(c3));   // all four in registers here: issued together, none deferred into a branch
      const bool g1 = key >= c1, g2 = key >= c2, g3 = key >= c3;
      esel = g2 ? c2 : (g1 ? c1 : c0);
      lo += (g1 ? 1u : 0u) + (g2 ? 1u : 0u);
      if (!__ballot(g3)) break;                              // a lane that has its symbol finds it again: c0 = its entry, g1 false
      lo += g3 ? 1u : 0u;
    }
    const unsigned xn = ((esel & 0xffffu) + 1u) * (x >> 16) + slot - (esel >> 16);
    x = active ? xn : x;                                     // a lane without an element keeps its state (always >= 2^16)
    const bool need = x < (1u << 16);
    const unsigned long long mask = __ballot(need);          // one word each, in lane order, from the shared pointer
    {
      const int q = R.ptr + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u));
      const unsigned word = R.ring[q & (kWordRing - 1)];
      x = need ? ((x << 16) | word) : x;
      R.ptr += __popcll(mask);
    }
    const int n = (int)(m.y >> 16), vmin = (int)(short)(m.y & 0xffffu);
    int v = (int)lo + vmin;
    const bool esc = active && (int)lo == n - 1;
    const unsigned long long emask = __ballot(esc);
    if (emask) {
      const int q = R.ptr + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(emask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)emask, 0u));
      const unsigned word = R.ring[q & (kWordRing - 1)];
      v = esc ? (int)(x & 0xffffu) - 32768 : v;
      x = esc ? ((x & 0xffff0000u) | word) : x;
      R.ptr += __popcll(emask);
    }
    return v;
  }
};

// One wave per stream, as the encoder.
template <class Search, class Src>
__device__ __forceinline__ void rans_decode_body(const unsigned short* __restrict__ payload, const long long* __restrict__ offsets,
                                                 Src& src, int segs, int L, long long E, long long Eseg,
                                                 const typename Search::Tables& T, int* __restrict__ bad) {
  extern __shared__ unsigned char smem[];
  Search S;
  S.stage(T, smem + Src::kStaging);
  const int s = blockIdx.x, lane = threadIdx.x;
  const RansStream st = rans_stream(s, segs, L, E, Eseg);
  const unsigned short* w = payload + offsets[s];
  const long long len = offsets[s + 1] - offsets[s];
  if (len < 2 * L || len > 0x3fffffff) {                     // not even the lane states, or longer than any encoder writes
    if (lane == 0) atomicAdd(bad, 1);
    return;
  }
  unsigned x = lane < L ? (((unsigned)w[2 * lane] << 16) | w[2 * lane + 1]) : (1u << 16);
  WordRing R{w, src.init(st, L, lane, smem), (int)len, lane, 2 * L, 2 * L, 2 * L, 2 * L, {}};
  R.fetch(R.ptr + kWordRing / 2);
  R.spill();
  R.fetch(R.ptr + kWordRing);
  R.spill();
  src.fetch(0);
  src.spill(0);

  typename Search::Desc m1;
  src.start(S.desc, m1);
  auto step = [&](auto full_tag, typename Src::Out* vout, int i, int cnt) {
    constexpr bool FULL = decltype(full_tag)::value;         // no per-lane "active" selects, no store predicate
    const bool active = FULL || src.active();
    const typename Search::Desc m = m1;
    src.template advance<FULL>(i, cnt, S.desc, m1);
    const int v = S.step(active, m, x, R);
    if (active) vout[i * L] = (typename Src::Out)v;
  };
  for (int k = 0; k < st.nchunks; ++k) {
    src.fetch(k + 1);
    R.fetch(R.ptr + kWordRing);
    const int cnt = std::min(kChunk, st.steps - k * kChunk);
    typename Src::Out* vout = src.out + st.e0 + (long long)k * kChunk * L + lane;
    src.chunk(k, cnt, S.desc, m1);
    if (L == 64 && (k + 1) * kChunk * 64 <= st.n) {          // all chunks but a stream's last, with 64 lanes
#pragma unroll
      for (int i = 0; i < kChunk; ++i) step(std::true_type{}, vout, i, kChunk);
    } else {
      for (int i = 0; i < cnt; ++i) step(std::false_type{}, vout, i, cnt);
    }
    R.spill();
    src.spill(k + 1);
  }
  // a well-formed stream ends with every state back at its initial value and the pointer at the end
  const bool good = S.qmax < R.len && x == (1u << 16) && R.ptr == R.len;
  if (__ballot(!good) && lane == 0) atomicAdd(bad, 1);
}

}  // namespace sntc

// ---- host side of the launches, shared by the extern "C" pairs of rans.hip and rans_channels.hip

// start-table entries that fit next to the rings, the descriptors and the packed decoder entries
static inline long long rans_lut_budget(int staging, int ntables, int total_entries) {
  const long long dec_bytes = 4LL * (((long long)total_entries + 3LL * ntables + 3) / 4 * 4);
  const long long rest = (long long)(sntc::kRansLdsTotal - staging) - (long long)ntables * (long long)sizeof(uint4) - dec_bytes;
  return rest < 16 ? 0 : rest / 2 / 8 * 8;
}

// Launches `in_lds` with the tables staged behind the rings where they fit, else `in_global`, which reads them where they are.
template <class... P, class... A>
static int rans_launch(void (*in_lds)(P...), void (*in_global)(P...), int staging, const sntc::RansTables& T, int nstreams,
                       hipStream_t s, A... args) {
  const int tb = sntc::rans_table_bytes(T.ntables, T.total);
  if (tb <= sntc::kRansLdsTotal - staging) {
    SNTC_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(in_lds), hipFuncAttributeMaxDynamicSharedMemorySize, staging + tb));
    hipLaunchKernelGGL(in_lds, dim3(nstreams), dim3(64), staging + tb, s, args...);
  } else {
    hipLaunchKernelGGL(in_global, dim3(nstreams), dim3(64), staging, s, args...);
  }
  SNTC_HIP(hipGetLastError());
  return SNTC_OK;
}

// The decoder's own tables as `who` (an entry point) was given them: dec / lut / lut_meta come together or not at all, and
// lut_entries covers every table, is a multiple of 8 and within rans_lut_budget().  -> D (D.dec == nullptr: none were given) and
// the dynamic LDS of the start-table kernel.
static int rans_dec_tables(const char* who, int staging, const uint32_t* dec, const uint16_t* lut, const uint32_t* meta,
                           const uint32_t* lut_meta, int ntables, int total_entries, int lut_entries, sntc::RansDecTables& D, int& lds) {
  const bool fast = dec != nullptr;
  if (fast != (lut != nullptr) || fast != (lut_meta != nullptr) ||
      (fast && (lut_entries < ntables || (lut_entries & 7) || lut_entries > rans_lut_budget(staging, ntables, total_entries))))
    return sntc::fail(SNTC_ERR_BAD_SHAPE, std::string(who) + ": dec / lut / lut_meta come together, lut_entries a multiple of 8 within the "
                                                             "LDS left beside the rings (sntc_rans_lut_budget() entries always are)");
  D = sntc::RansDecTables{};
  lds = 0;
  if (fast) {
    const int dec_total = (total_entries + 3 * ntables + 3) / 4 * 4;        // within the budget checked above: no overflow
    D = sntc::RansDecTables{dec, lut, reinterpret_cast<const uint2*>(meta), lut_meta, ntables, dec_total, lut_entries};
    lds = staging + ntables * (int)sizeof(uint4) + dec_total * 4 + lut_entries * 2;
  }
  return SNTC_OK;
}
