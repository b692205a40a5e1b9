// rans_channels.hip -- the rANS coder of rans.hip for "one latent, table = channel": the latents of the factorized-prior
// model (reference factorized/models.py:101-124, whose entropy model is one deep-factorized density per channel).
//
// Same streams, word for word, as rans.hip codes for the same values with table id = channel (format: the head of rans.hip).
// What differs is what a wave touches around the coding loop:
//   * no table-id tensor: element e of an image (flat NHWC) has table e % C.  A lane's element index grows by L per step, so
//     its table id advances by L % C with one conditional subtract -- no division in the loop, no id ring in LDS (its 4 KB go
//     to the tables);
//   * the encoder reads the float latents and rounds them itself (rintf: half to even, what round_to_int_kernel and the
//     prior scan's y_hat do) and can write the rounded latents on the way; the decoder writes floats: no int32 tensor.
#include <algorithm>
#include <type_traits>
#include "rans_common.h"

namespace sntc {

// staging: the encoder's value ring [2][kChunk * 64] int, or the decoder's word ring [kWordRing] uint16 -- both 8 KB
constexpr int kChanStagingBytes = 2 * kChunk * 64 * 4;
static_assert(kWordRing * 2 <= kChanStagingBytes, "decoder ring must fit the staging area");
constexpr int kChanLdsLimit = kRansLdsTotal - kChanStagingBytes;   // what the tables may take

// what every kernel here derives from its block index: stream s = (image b, segment sg) codes elements [e0, e0 + n) of y, and
// the table of its element r is (tbase + r) % C  (E % C == 0, so an image's first element is channel 0)
struct ChanStream {
  long long e0;
  int n, steps, tbase, lstep;
};

__device__ __forceinline__ ChanStream chan_stream(int s, int segs, int L, int C, long long E, long long Eseg) {
  const int b = s / segs, sg = s - b * segs;
  const long long r0 = (long long)sg * Eseg;
  const long long r1 = std::min(E, r0 + Eseg);
  ChanStream st;
  st.e0 = (long long)b * E + r0;
  st.n = r1 > r0 ? (int)(r1 - r0) : 0;                       // host: cap_words < 2^30, so a segment's elements fit 32 bits
  st.steps = (st.n + L - 1) / L;
  st.tbase = (int)(r0 % C);
  st.lstep = L % C;
  return st;
}

// one wave per stream, as rans_encode_kernel
template <bool LDS>
__global__ void __launch_bounds__(64) rans_encode_channels_kernel(const float* __restrict__ y, int segs, int L, int C, long long E,
                                                                  long long Eseg, RansTables T, long long cap,
                                                                  unsigned short* __restrict__ scratch, int* __restrict__ len_words,
                                                                  float* __restrict__ y_hat) {
  extern __shared__ unsigned char smem[];
  int* vring = reinterpret_cast<int*>(smem);                                         // [2][kChunk * 64]
  const uint2* meta;
  const unsigned short* cdf;
  rans_stage_tables<LDS>(T, smem + kChanStagingBytes, meta, cdf);
  const int s = blockIdx.x, lane = threadIdx.x;
  const ChanStream st = chan_stream(s, segs, L, C, E, Eseg);
  const int steps = st.steps, nchunks = (steps + kChunk - 1) / kChunk;
  unsigned short* out = scratch + (size_t)s * cap;
  long long wp = cap;
  const unsigned long long gt = lane == 63 ? 0ull : (~0ull << (lane + 1));
  unsigned x = 1u << 16;
  const int nl = lane < L ? st.n : 0;                        // the lane has an element at position r of the stream iff r < nl

  // the floats stay in registers, untouched, while the chunk before them is coded (their loads are in flight meanwhile);
  // they are rounded, and written back as y_hat, when they are dropped into the ring
  float FR[kChunk];
  auto fetch = [&](int k) {
#pragma unroll
    for (int i = 0; i < kChunk; ++i) {
      const int r = (k * kChunk + i) * L + lane;
      FR[i] = (k >= 0 && r < nl) ? y[st.e0 + r] : 0.0f;
    }
  };
  auto spill = [&](int k) {
#pragma unroll
    for (int i = 0; i < kChunk; ++i) {
      const int v = (int)rintf(FR[i]);
      vring[(k & 1) * kChunk * 64 + i * 64 + lane] = v;
      const int r = (k * kChunk + i) * L + lane;
      if (y_hat && k >= 0 && r < nl) y_hat[st.e0 + r] = (float)v;
    }
  };
  struct Sym { unsigned f, c, raw; bool active, esc; };
  auto lookup = [&](int t, int v, uint2 m) -> Sym {
    const bool active = t != kNoTable;
    const int n = (int)(m.y >> 16);
    bool esc;
    int sym = rans_symbol(v, m, esc);
    esc = active && esc;
    if (!active) sym = 0;
    const unsigned cl = cdf[m.x + sym];
    const unsigned ch = sym + 1 < n ? (unsigned)cdf[m.x + sym + 1] : 65536u;
    return Sym{active ? ch - cl : 1u, cl, (unsigned)(std::min(std::max(v, -32768), 32767) + 32768), active, esc};
  };
  // the steps are read in strictly descending order (last step of the last chunk first), so the lane carries the position
  // rq and the table id tq of the next step to read: -L and -(L % C) with a wrap per step
  int rq = (steps - 1) * L + lane;
  int tq = steps > 0 ? (int)(((long long)st.tbase + rq) % C) : 0;
  if (nchunks > 0) {
    fetch(nchunks - 1);
    spill(nchunks - 1);
  }
  for (int k = nchunks - 1; k >= 0; --k) {
    fetch(k - 1);
    const int buf = k & 1;
    const int* vb = vring + buf * kChunk * 64 + lane;
    const int cnt = std::min(kChunk, steps - k * kChunk);
    auto rd = [&](int i, int& t, int& v) {
      if (i < 0) {
        t = kNoTable;
        v = 0;
        return;
      }
      t = rq < nl ? tq : (int)kNoTable;
      v = vb[i * 64];
      rq -= L;
      tq -= st.lstep;
      tq += tq < 0 ? C : 0;
    };
    int t1, v1, t2, v2;
    rd(cnt - 1, t1, v1);
    Sym cur = lookup(t1, v1, meta[t1 == kNoTable ? 0 : t1]);
    rd(cnt - 2, t1, v1);
    uint2 m1 = meta[t1 == kNoTable ? 0 : t1];
    rd(cnt - 3, t2, v2);
    for (int i = cnt - 1; i >= 0; --i) {
      const Sym sy = cur;
      cur = lookup(t1, v1, m1);                             // step i - 1
      t1 = t2;
      v1 = v2;
      m1 = meta[t1 == kNoTable ? 0 : t1];                   // step i - 2
      rd(i - 3, t2, v2);
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
    spill(k - 1);
  }
  wp -= 2 * L;
  if (lane < L) {
    out[wp + 2 * lane] = (unsigned short)(x >> 16);
    out[wp + 2 * lane + 1] = (unsigned short)(x & 0xffffu);
  }
  if (lane == 0) len_words[s] = (int)(cap - wp);
}

// The decoder's stream words: the ring holds [ptr, ptr + kWordRing) at the start of a chunk; a chunk eats at most kWordRing / 2.
// Stream positions fit 32 bits (host: cap_words < 2^30).
struct WordRing {
  const unsigned short* w;
  unsigned short* ring;
  int len, lane, filled, wfrom, wto;
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

// binary search of cdf per symbol (tables in LDS, or in global memory where they do not fit), as rans_decode_kernel
template <bool LDS>
__global__ void __launch_bounds__(64) rans_decode_channels_kernel(const unsigned short* __restrict__ payload,
                                                                  const long long* __restrict__ offsets, int segs, int L, int C,
                                                                  long long E, long long Eseg, RansTables T, float* __restrict__ y_hat,
                                                                  int* __restrict__ bad) {
  extern __shared__ unsigned char smem[];
  const uint2* meta;
  const unsigned short* cdf;
  rans_stage_tables<LDS>(T, smem + kChanStagingBytes, meta, cdf);
  const int s = blockIdx.x, lane = threadIdx.x;
  const ChanStream st = chan_stream(s, segs, L, C, E, Eseg);
  const int steps = st.steps, nchunks = (steps + kChunk - 1) / kChunk;
  const unsigned short* w = payload + offsets[s];
  const long long len = offsets[s + 1] - offsets[s];
  if (len < 2 * L || len > 0x3fffffff) {                     // not even the lane states, or longer than any encoder writes
    if (lane == 0) atomicAdd(bad, 1);
    return;
  }
  unsigned x = lane < L ? (((unsigned)w[2 * lane] << 16) | w[2 * lane + 1]) : (1u << 16);
  bool ok = true;
  const unsigned long long lt = (1ull << lane) - 1ull;
  int ptr = 2 * L;
  WordRing R{w, reinterpret_cast<unsigned short*>(smem), (int)len, lane, 2 * L, 2 * L, 2 * L, {}};
  const unsigned short* wring = R.ring;
  const int len32 = R.len;
  R.fetch(ptr + kWordRing / 2);
  R.spill();
  R.fetch(ptr + kWordRing);
  R.spill();

  // the lane's position in the stream and its table id, step by step: +L and +(L % C) with a wrap
  const int nl = lane < L ? st.n : 0;                        // the lane has an element at position r iff r < nl
  int rq = lane;
  int t1 = (st.tbase + lane) % C;
  uint2 m1 = meta[t1];
  // One step.  FULL: every lane has an element in every step of the chunk (all chunks but a stream's last, with 64 lanes) -- no
  // per-lane "active" selects, no store predicate.
  auto step = [&](auto full_tag, float* vout, int i) {
    constexpr bool FULL = decltype(full_tag)::value;
    const bool active = FULL || rq < nl;
    const uint2 m = m1;
    rq += L;
    t1 += st.lstep;
    t1 -= t1 >= C ? C : 0;
    m1 = meta[t1];                                           // descriptor of the next step
    const int n = active ? (int)(m.y >> 16) : 1, vmin = (int)(short)(m.y & 0xffffu);
    const unsigned short* c = cdf + m.x;
    const unsigned slot = x & 0xffffu;
    // the largest sym with cdf[sym] <= slot; the bracketing cdf values are carried along so that no read follows the search
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
    if (active) x = (chi - clo) * (x >> 16) + slot - clo;
    const bool need = active && x < (1u << 16);
    const unsigned long long mask = __ballot(need);
    if (mask) {                                              // one word each, in lane order, from the shared pointer
      if (need) {
        const int q = ptr + __popcll(mask & lt);
        ok &= q < len32;
        x = (x << 16) | wring[q & (kWordRing - 1)];
      }
      ptr += __popcll(mask);
    }
    int v = lo + vmin;
    const bool esc = active && lo == n - 1;
    const unsigned long long emask = __ballot(esc);
    if (emask) {
      if (esc) {
        const int q = ptr + __popcll(emask & lt);
        ok &= q < len32;
        v = (int)(x & 0xffffu) - 32768;
        x = (x & 0xffff0000u) | wring[q & (kWordRing - 1)];
      }
      ptr += __popcll(emask);
    }
    if (active) vout[(long long)i * L] = (float)v;
  };
  for (int k = 0; k < nchunks; ++k) {
    R.fetch(ptr + kWordRing);
    const int cnt = std::min(kChunk, steps - k * kChunk);
    float* vout = y_hat + st.e0 + (long long)k * kChunk * L + lane;
    if (L == 64 && (k + 1) * kChunk * 64 <= st.n) {
      for (int i = 0; i < kChunk; ++i) step(std::true_type{}, vout, i);
    } else {
      for (int i = 0; i < cnt; ++i) step(std::false_type{}, vout, i);
    }
    R.spill();
  }
  // a well-formed stream ends with every state back at its initial value and the pointer at the end
  const bool good = ok && x == (1u << 16) && ptr == len32;
  if (__ballot(!good) && lane == 0) atomicAdd(bad, 1);
}

// the decoder's own tables (RansDecTables) in LDS, as rans_decode_fast_kernel: start symbol from the start table, four
// consecutive entries from there, refill word -- three LDS round trips per step
__global__ void __launch_bounds__(64) rans_decode_channels_fast_kernel(const unsigned short* __restrict__ payload,
                                                                       const long long* __restrict__ offsets, int segs, int L, int C,
                                                                       long long E, long long Eseg, RansDecTables T,
                                                                       float* __restrict__ y_hat, int* __restrict__ bad) {
  extern __shared__ unsigned char smem[];
  uint4* m4 = reinterpret_cast<uint4*>(smem + kChanStagingBytes);                    // {entry offset, n | vmin, lut offset, 16 - bits}
  unsigned* dec = reinterpret_cast<unsigned*>(m4 + T.ntables);
  unsigned short* lut = reinterpret_cast<unsigned short*>(dec + T.dec_total);
  const int lane = threadIdx.x;
  for (int i = lane; i < T.ntables; i += 64) {
    const uint2 a = T.meta[i];
    const unsigned lm = T.lmeta[i];
    m4[i] = make_uint4(a.x + 3u * (unsigned)i, a.y, lm >> 5, 16u - (lm & 31u));
  }
  {
    const uint4* src = reinterpret_cast<const uint4*>(T.dec);
    uint4* dst = reinterpret_cast<uint4*>(dec);
    for (int i = lane; i < T.dec_total / 4; i += 64) dst[i] = src[i];
    src = reinterpret_cast<const uint4*>(T.lut);
    dst = reinterpret_cast<uint4*>(lut);
    for (int i = lane; i < T.lut_total / 8; i += 64) dst[i] = src[i];
  }
  __syncthreads();
  const int s = blockIdx.x;
  const ChanStream st = chan_stream(s, segs, L, C, E, Eseg);
  const int steps = st.steps, nchunks = (steps + kChunk - 1) / kChunk;
  const unsigned short* w = payload + offsets[s];
  const long long len = offsets[s + 1] - offsets[s];
  if (len < 2 * L || len > 0x3fffffff) {                     // not even the lane states, or longer than any encoder writes
    if (lane == 0) atomicAdd(bad, 1);
    return;
  }
  unsigned x = lane < L ? (((unsigned)w[2 * lane] << 16) | w[2 * lane + 1]) : (1u << 16);
  int ptr = 2 * L;
  WordRing R{w, reinterpret_cast<unsigned short*>(smem), (int)len, lane, 2 * L, 2 * L, 2 * L, {}};
  const unsigned short* wring = R.ring;
  const int len32 = R.len;
  R.fetch(ptr + kWordRing / 2);
  R.spill();
  R.fetch(ptr + kWordRing);
  R.spill();

  const int nl = lane < L ? st.n : 0;                        // the lane has an element at position r iff r < nl
  int rq = lane;
  int t1 = (st.tbase + lane) % C;
  uint4 m1 = m4[t1];
  // One step.  FULL: every lane has an element in every step of the chunk (all chunks but a stream's last, with 64 lanes) -- no
  // per-lane "active" selects, no store predicate.  A word index at or past the stream's end is not checked here: the
  // pointer only grows, so it ends past the length and the stream is counted as bad below; the ring read itself is masked.
  auto step = [&](auto full_tag, float* vout, int i) {
    constexpr bool FULL = decltype(full_tag)::value;
    const bool active = FULL || rq < nl;
    const uint4 m = m1;
    rq += L;
    t1 += st.lstep;
    t1 -= t1 >= C ? C : 0;
    m1 = m4[t1];                                             // descriptor of the next step
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
      const int q = ptr + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u));
      const unsigned word = wring[q & (kWordRing - 1)];
      x = need ? ((x << 16) | word) : x;
      ptr += __popcll(mask);
    }
    const int n = (int)(m.y >> 16), vmin = (int)(short)(m.y & 0xffffu);
    int v = (int)lo + vmin;
    const bool esc = active && (int)lo == n - 1;
    const unsigned long long emask = __ballot(esc);
    if (emask) {
      const int q = ptr + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(emask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)emask, 0u));
      const unsigned word = wring[q & (kWordRing - 1)];
      v = esc ? (int)(x & 0xffffu) - 32768 : v;
      x = esc ? ((x & 0xffff0000u) | word) : x;
      ptr += __popcll(emask);
    }
    if (active) vout[(long long)i * L] = (float)v;
  };

  for (int k = 0; k < nchunks; ++k) {
    R.fetch(ptr + kWordRing);
    const int cnt = std::min(kChunk, steps - k * kChunk);
    float* vout = y_hat + st.e0 + (long long)k * kChunk * L + lane;
    if (L == 64 && (k + 1) * kChunk * 64 <= st.n) {
#pragma unroll
      for (int i = 0; i < kChunk; ++i) step(std::true_type{}, vout, i);
    } else {
      for (int i = 0; i < cnt; ++i) step(std::false_type{}, vout, i);
    }
    R.spill();
  }
  const bool good = x == (1u << 16) && ptr == len32;
  if (__ballot(!good) && lane == 0) atomicAdd(bad, 1);
}

}  // namespace sntc

using namespace sntc;

static int chan_sizes_ok(int nimages, int64_t elems_per_image, int channels, int segments, int lanes, int total_entries) {
  return nimages >= 1 && elems_per_image >= 1 && channels >= 1 && channels < (int)kNoTable && elems_per_image % channels == 0 &&
         segments >= 1 && rans_lanes_ok(lanes) && total_entries >= 1;
}

extern "C" int sntc_rans_encode_channels(const float* y, int nimages, int64_t elems_per_image, int channels, int segments, int lanes,
                                         const uint16_t* cdf, const uint32_t* meta, int total_entries, int64_t cap_words,
                                         uint16_t* scratch, int32_t* len_words, float* y_hat, void* stream) {
  if (!y || !cdf || !meta || !scratch || !len_words) return fail(SNTC_ERR_BAD_SHAPE, "sntc_rans_encode_channels: null argument");
  if (!chan_sizes_ok(nimages, elems_per_image, channels, segments, lanes, total_entries) ||
      cap_words < sntc_rans_cap_words(elems_per_image, segments) || cap_words > 0x3fffffff)
    return fail(SNTC_ERR_BAD_SHAPE, "sntc_rans_encode_channels: bad sizes (elems_per_image a multiple of channels, cap_words >= "
                                    "sntc_rans_cap_words())");
  const RansTables T{cdf, reinterpret_cast<const uint2*>(meta), channels, total_entries};
  const long long eseg = rans_segment_elems(elems_per_image, segments);
  const int ns = nimages * segments, tb = rans_table_bytes(channels, total_entries), lds = kChanStagingBytes + tb;
  hipStream_t s = (hipStream_t)stream;
  if (tb <= kChanLdsLimit) {
    SNTC_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(rans_encode_channels_kernel<true>),
                                 hipFuncAttributeMaxDynamicSharedMemorySize, lds));
    hipLaunchKernelGGL(rans_encode_channels_kernel<true>, dim3(ns), dim3(64), lds, s, y, segments, lanes, channels,
                       (long long)elems_per_image, eseg, T, (long long)cap_words, scratch, len_words, y_hat);
  } else {
    hipLaunchKernelGGL(rans_encode_channels_kernel<false>, dim3(ns), dim3(64), kChanStagingBytes, s, y, segments, lanes, channels,
                       (long long)elems_per_image, eseg, T, (long long)cap_words, scratch, len_words, y_hat);
  }
  SNTC_HIP(hipGetLastError());
  return SNTC_OK;
}

extern "C" int sntc_rans_decode_channels(const uint16_t* payload, const int64_t* offsets, int nimages, int64_t elems_per_image,
                                         int channels, int segments, int lanes, const uint16_t* cdf, const uint32_t* meta,
                                         int total_entries, const uint32_t* dec, const uint16_t* lut, const uint32_t* lut_meta,
                                         int lut_entries, float* y_hat, int32_t* bad_streams, void* stream) {
  if (!payload || !offsets || !cdf || !meta || !y_hat || !bad_streams)
    return fail(SNTC_ERR_BAD_SHAPE, "sntc_rans_decode_channels: null argument");
  if (!chan_sizes_ok(nimages, elems_per_image, channels, segments, lanes, total_entries) ||
      sntc_rans_cap_words(elems_per_image, segments) > 0x3fffffff)
    return fail(SNTC_ERR_BAD_SHAPE, "sntc_rans_decode_channels: bad sizes (elems_per_image a multiple of channels)");
  const bool fast = dec != nullptr;
  const long long dec_total = ((long long)total_entries + 3LL * channels + 3) / 4 * 4;
  const long long fast_lds = (long long)kChanStagingBytes + (long long)channels * (long long)sizeof(uint4) + dec_total * 4 + (long long)lut_entries * 2;
  if (fast != (lut != nullptr) || fast != (lut_meta != nullptr) ||
      (fast && (lut_entries < channels || (lut_entries & 7) || fast_lds > kRansLdsTotal)))
    return fail(SNTC_ERR_BAD_SHAPE, "sntc_rans_decode_channels: dec / lut / lut_meta come together, lut_entries a multiple of 8, the "
                                    "decoder's tables within a CU's LDS (sntc_rans_lut_budget() entries always are)");
  const long long eseg = rans_segment_elems(elems_per_image, segments);
  const int ns = nimages * segments;
  hipStream_t s = (hipStream_t)stream;
  if (int zrc = zero_async(bad_streams, sizeof(int32_t), s)) return zrc;
  const long long* offs = reinterpret_cast<const long long*>(offsets);
  if (fast) {
    const RansDecTables D{dec, lut, reinterpret_cast<const uint2*>(meta), lut_meta, channels, (int)dec_total, lut_entries};
    SNTC_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(rans_decode_channels_fast_kernel),
                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)fast_lds));
    hipLaunchKernelGGL(rans_decode_channels_fast_kernel, dim3(ns), dim3(64), (int)fast_lds, s, payload, offs, segments, lanes, channels,
                       (long long)elems_per_image, eseg, D, y_hat, bad_streams);
    SNTC_HIP(hipGetLastError());
    return SNTC_OK;
  }
  const RansTables T{cdf, reinterpret_cast<const uint2*>(meta), channels, total_entries};
  const int tb = rans_table_bytes(channels, total_entries), lds = kChanStagingBytes + tb;
  if (tb <= kChanLdsLimit) {
    SNTC_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(rans_decode_channels_kernel<true>),
                                 hipFuncAttributeMaxDynamicSharedMemorySize, lds));
    hipLaunchKernelGGL(rans_decode_channels_kernel<true>, dim3(ns), dim3(64), lds, s, payload, offs, segments, lanes, channels,
                       (long long)elems_per_image, eseg, T, y_hat, bad_streams);
  } else {
    hipLaunchKernelGGL(rans_decode_channels_kernel<false>, dim3(ns), dim3(64), kChanStagingBytes, s, payload, offs, segments, lanes,
                       channels, (long long)elems_per_image, eseg, T, y_hat, bad_streams);
  }
  SNTC_HIP(hipGetLastError());
  return SNTC_OK;
}
