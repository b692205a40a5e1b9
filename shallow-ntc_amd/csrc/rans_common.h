// rans_common.h -- what the rANS translation units share: the table views, the symbol of a value, the staging constants and
// the host-side stream arithmetic.  rans.hip codes with a table id per element and rans_channels.hip with table = channel, from /
// to floats: both instantiate the one coder of rans_kernel.h; rans_cost.hip sums what the coded symbols cost.
// The stream format is described once, at the head of rans.hip.
#pragma once
#include "sntc_internal.h"

namespace sntc {

struct RansTables {
  const unsigned short* cdf;   // concatenated; table t: cdf[off .. off + n), cdf of symbol n (= 65536) implicit
  const uint2* meta;           // per table: x = off, y = (n << 16) | (vmin & 0xffff); symbol n-1 is ESCAPE
  int ntables;
  int total;                   // entries in cdf
};

// The decoder's own view of the same tables (optional: sntc_rans_decode's dec / lut arguments, built by the host from cdf):
//   dec  entry s of table t, at dec[off_t + 3 t + s] = (cdf[s] << 16) | (freq[s] - 1), followed by three 0xffffffff -- ONE read
//        gives a symbol's (start, frequency), and with key = (slot << 16) | 0xfffe, "key >= entry" is "slot >= cdf[s]" for every
//        real entry (freq - 1 <= 0xfffe: a table has >= 2 symbols) and false for the sentinels;
//   lut  per table a START TABLE of 2^bits entries, lut[lut_off + (slot >> (16 - bits))] = the largest symbol whose cdf is <= the
//        first slot of that bucket: the search starts there.  lmeta[t] = (lut_off << 5) | bits.
struct RansDecTables {
  const unsigned* dec;
  const unsigned short* lut;
  const uint2* meta;           // RansTables::meta
  const unsigned* lmeta;
  int ntables;
  int dec_total;               // entries in dec: total + 3 * ntables, padded to a multiple of 4
  int lut_total;               // entries in lut, padded to a multiple of 8
};

// Staging.  A wave that codes one stream has nobody to hide memory latency behind, so nothing in the coding loops
// touches global memory for input: table ids (and values / stream words) are fetched a CHUNK of 16 steps ahead into
// registers and dropped into LDS rings when the chunk ends; the loops read LDS only, one to two steps ahead of use.
constexpr int kChunk = 16;                        // steps per staging chunk (1024 elements)
constexpr int kWordRing = 4096;                   // decoder: stream words resident in LDS (2 x the most a chunk can eat)
constexpr int kWordRegs = 2 * kChunk;             // decoder: words one lane fetches per chunk
constexpr int kRansLdsTotal = 150 * 1024;         // dynamic LDS one coding workgroup asks for at the most: rings + tables
constexpr unsigned short kNoTable = 0xffffu;      // ring entry of a lane with no element in that step

template <bool LDS>
__device__ __forceinline__ void rans_stage_tables(const RansTables& T, unsigned char* smem, const uint2*& meta,
                                                  const unsigned short*& cdf) {
  if (LDS) {
    uint2* m = reinterpret_cast<uint2*>(smem);
    unsigned short* c = reinterpret_cast<unsigned short*>(smem + (size_t)T.ntables * sizeof(uint2));
    for (int i = threadIdx.x; i < T.ntables; i += blockDim.x) m[i] = T.meta[i];
    const unsigned* src = reinterpret_cast<const unsigned*>(T.cdf);   // host pads the table to an even count
    unsigned* dst = reinterpret_cast<unsigned*>(c);
    for (int i = threadIdx.x; i < (T.total + 1) / 2; i += blockDim.x) dst[i] = src[i];
    __syncthreads();
    meta = m;
    cdf = c;
  } else {
    meta = T.meta;
    cdf = T.cdf;
  }
}

// The symbol a value takes in the table of descriptor m (RansTables::meta): v - vmin where that is one of the table's n - 1
// real symbols, else ESCAPE (the last symbol, n - 1; the value itself then travels as a raw 16-bit word).  The encoders code
// this symbol and sntc_rans_cost prices it: one definition, so the price is that of the word stream.
__device__ __forceinline__ int rans_symbol(int v, uint2 m, bool& esc) {
  const int n = (int)(m.y >> 16), vmin = (int)(short)(m.y & 0xffffu);
  const int sym = v - vmin;
  esc = sym < 0 || sym >= n - 1;
  return esc ? n - 1 : sym;
}

// elements of one segment: an image's elements cut into `segments` runs, each a multiple of 64
static inline long long rans_segment_elems(long long elems, int segments) {
  const long long per = (elems + segments - 1) / segments;
  return (per + 63) / 64 * 64;
}

static inline int rans_table_bytes(int ntables, int total) { return ntables * (int)sizeof(uint2) + ((total + 1) / 2) * 4; }

static inline bool rans_lanes_ok(int lanes) { return lanes == 8 || lanes == 16 || lanes == 32 || lanes == 64; }

}  // namespace sntc
