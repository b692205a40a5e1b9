// rans.hip -- the bitstream behind the rate estimates: table-driven, 64-way interleaved rANS.
//
// The reference always runs its entropy models with compression=False (mshyper/models.py:246-251) and reports
// the *estimated* rate; this coder is this build's own wire format, not TFC's.
//
// One stream per (image, segment); ONE WAVE codes a stream: the segment's elements (flat [P, C] order) are dealt
// round-robin to L = 8 .. 64 lanes (step j, lane l <-> element L j + l, so table-id / value accesses are one coalesced
// line per step), every lane owns a 32-bit rANS state and all lanes share one sequence of 16-bit words:
//   decode step:  s = x & 0xffff -> (symbol, f, c);  x = f (x >> 16) + s - c;  lanes with x < 2^16 each take ONE
//                 word, in lane order, from the shared read pointer (wave ballot + popcount of lower lanes);
//                 lanes whose symbol was ESCAPE then read the value: v = (x & 0xffff) - 32768, x >>= 16, and
//                 refill the same way (a second, usually empty, sub-step).
//   encode step:  the exact mirror, steps in reverse, writing backward: ESCAPE lanes emit x & 0xffff and set
//                 x = (x & ~0xffff) | (v + 32768); then lanes with x >= f << 16 emit x & 0xffff, x >>= 16;
//                 x = ((x / f) << 16) + x % f + c.  The highest lane gets the highest address.
//   stream     =  [L x (state hi, state lo)] [words in decode order]; every state starts (encoder) and must end
//                 (decoder) at 2^16, and the read pointer must end at the stream's length: a free integrity check.
// Cost of the parallelism: 4 L bytes of flushed state per stream (the host uses fewer lanes on short streams).  Probability precision 16 bits; CDF tables are
// uint16 (cdf[n] = 65536 implicit) and live in LDS next to a packed (offset, n, vmin) descriptor per table.
#include "rans_kernel.h"

namespace sntc {

// the coder of rans_kernel.h on a table id per element (IdEnc / IdDec): LDS = the tables staged in LDS, else read from global memory
template <bool LDS>
__global__ void __launch_bounds__(64) rans_encode_kernel(const int* __restrict__ values, const unsigned short* __restrict__ tid,
                                                         int segs, int L, long long E, long long Eseg, RansTables T, long long cap,
                                                         unsigned short* __restrict__ scratch, int* __restrict__ len_words) {
  IdEnc src;
  src.values = values;
  src.tid = tid;
  rans_encode_body<LDS>(src, segs, L, E, Eseg, T, cap, scratch, len_words);
}

__global__ void rans_compact_kernel(const unsigned short* __restrict__ src, long long cap, const int* __restrict__ len_words,
                                    const long long* __restrict__ offsets, int nstreams, unsigned short* __restrict__ dst) {
  const int s = blockIdx.x;
  if (s >= nstreams) return;
  const int len = len_words[s];
  const unsigned short* from = src + (size_t)(s + 1) * cap - len;
  unsigned short* to = dst + offsets[s];
  for (int i = threadIdx.x; i < len; i += blockDim.x) to[i] = from[i];
}

template <bool LDS>
__global__ void __launch_bounds__(64) rans_decode_kernel(const unsigned short* __restrict__ payload, const long long* __restrict__ offsets,
                                                         const unsigned short* __restrict__ tid, int segs, int L, long long E, long long Eseg,
                                                         RansTables T, int* __restrict__ values, int* __restrict__ bad) {
  IdDec src;
  src.tid = tid;
  src.out = values;
  rans_decode_body<CdfSearch<LDS>>(payload, offsets, src, segs, L, E, Eseg, T, bad);
}

__global__ void __launch_bounds__(64) rans_decode_fast_kernel(const unsigned short* __restrict__ payload, const long long* __restrict__ offsets,
                                                              const unsigned short* __restrict__ tid, int segs, int L, long long E,
                                                              long long Eseg, RansDecTables T, int* __restrict__ values,
                                                              int* __restrict__ bad) {
  IdDec src;
  src.tid = tid;
  src.out = values;
  rans_decode_body<StartTableSearch>(payload, offsets, src, segs, L, E, Eseg, T, bad);
}

// indexes = round(clamp(exp(raw), 0, 63)) as the table id of every y element (the integer scale table TFC's
// compress() path uses); raw = hyper[..., C:]
__global__ void scale_index_kernel(const float* __restrict__ hyper, long long npix, int c, unsigned short* __restrict__ tid) {
  const long long total = npix * c;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const long long p = i / c;
    const int ch = (int)(i - p * c);
    const float idx = fminf(fmaxf(expf(hyper[p * 2 * c + c + ch]), 0.0f), 63.0f);
    tid[i] = (unsigned short)rintf(idx);
  }
}

__global__ void channel_index_kernel(long long npix, int c, unsigned short* __restrict__ tid) {
  const long long total = npix * c;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x)
    tid[i] = (unsigned short)(i % c);
}

__global__ void round_to_int_kernel(const float* __restrict__ x, long long total, int* __restrict__ out) {
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x)
    out[i] = (int)rintf(x[i]);
}

__global__ void int_to_float_kernel(const int* __restrict__ x, long long total, float* __restrict__ out) {
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x)
    out[i] = (float)x[i];
}

}  // namespace sntc

using namespace sntc;

static int blocks_for(long long total) {
  long long b = (total + 255) / 256;
  return (int)(b < 1 ? 1 : (b > 2048 ? 2048 : b));
}

extern "C" int64_t sntc_rans_cap_words(int64_t elems_per_image, int segments) {
  if (elems_per_image < 1 || segments < 1) return -1;
  return 2 * rans_segment_elems(elems_per_image, segments) + 128;
}

extern "C" int sntc_rans_encode(const int32_t* values, const uint16_t* table_ids, int nimages, int64_t elems_per_image,
                                int segments, int lanes, const uint16_t* cdf, const uint32_t* meta, int ntables, int total_entries,
                                int64_t cap_words, uint16_t* scratch, int32_t* len_words, void* stream) {
  if (!values || !table_ids || !cdf || !meta || !scratch || !len_words)
    return fail(SNTC_ERR_BAD_SHAPE, "sntc_rans_encode: null argument");
  if (nimages < 1 || elems_per_image < 1 || segments < 1 || !rans_lanes_ok(lanes) || ntables < 1 || total_entries < 1 ||
      cap_words < sntc_rans_cap_words(elems_per_image, segments) || cap_words > 0x3fffffff)
    return fail(SNTC_ERR_BAD_SHAPE, "sntc_rans_encode: bad sizes (cap_words must be >= sntc_rans_cap_words())");
  const RansTables T{cdf, reinterpret_cast<const uint2*>(meta), ntables, total_entries};
  return rans_launch(rans_encode_kernel<true>, rans_encode_kernel<false>, kStagingBytes, T, nimages * segments, (hipStream_t)stream, values,
                     table_ids, segments, lanes, (long long)elems_per_image, rans_segment_elems(elems_per_image, segments), T,
                     (long long)cap_words, scratch, len_words);
}

extern "C" int sntc_rans_compact(const uint16_t* scratch, int64_t cap_words, const int32_t* len_words, const int64_t* offsets,
                                 int nstreams, uint16_t* payload, void* stream) {
  if (!scratch || !len_words || !offsets || !payload || nstreams < 1) return fail(SNTC_ERR_BAD_SHAPE, "sntc_rans_compact: bad argument");
  hipLaunchKernelGGL(rans_compact_kernel, dim3(nstreams), dim3(256), 0, (hipStream_t)stream, scratch, (long long)cap_words, len_words,
                     reinterpret_cast<const long long*>(offsets), nstreams, payload);
  SNTC_HIP(hipGetLastError());
  return SNTC_OK;
}

// start-table entries the id decoder has room for: what is left of a CU's LDS next to the staging rings, the descriptors and dec
extern "C" int64_t sntc_rans_lut_budget(int ntables, int total_entries) {
  if (ntables < 1 || total_entries < 1) return -1;
  return rans_lut_budget(kStagingBytes, ntables, total_entries);
}

extern "C" int sntc_rans_decode(const uint16_t* payload, const int64_t* offsets, const uint16_t* table_ids, int nimages,
                                int64_t elems_per_image, int segments, int lanes, const uint16_t* cdf, const uint32_t* meta,
                                int ntables, int total_entries, const uint32_t* dec, const uint16_t* lut, const uint32_t* lut_meta,
                                int lut_entries, int32_t* values, int32_t* bad_streams, void* stream) {
  if (!payload || !offsets || !table_ids || !cdf || !meta || !values || !bad_streams)
    return fail(SNTC_ERR_BAD_SHAPE, "sntc_rans_decode: null argument");
  if (nimages < 1 || elems_per_image < 1 || segments < 1 || !rans_lanes_ok(lanes) || ntables < 1 || total_entries < 1 ||
      sntc_rans_cap_words(elems_per_image, segments) > 0x3fffffff)
    return fail(SNTC_ERR_BAD_SHAPE, "sntc_rans_decode: bad sizes");
  RansDecTables D;
  int lds;
  if (int rc = rans_dec_tables("sntc_rans_decode", kStagingBytes, dec, lut, meta, lut_meta, ntables, total_entries, lut_entries, D, lds)) return rc;
  const long long eseg = rans_segment_elems(elems_per_image, segments);
  const int ns = nimages * segments;
  hipStream_t s = (hipStream_t)stream;
  if (int zrc = zero_async(bad_streams, sizeof(int32_t), s)) return zrc;
  const long long* offs = reinterpret_cast<const long long*>(offsets);
  if (D.dec) {
    SNTC_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(rans_decode_fast_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, lds));
    hipLaunchKernelGGL(rans_decode_fast_kernel, dim3(ns), dim3(64), lds, s, payload, offs, table_ids, segments, lanes,
                       (long long)elems_per_image, eseg, D, values, bad_streams);
    SNTC_HIP(hipGetLastError());
    return SNTC_OK;
  }
  const RansTables T{cdf, reinterpret_cast<const uint2*>(meta), ntables, total_entries};
  return rans_launch(rans_decode_kernel<true>, rans_decode_kernel<false>, kStagingBytes, T, ns, s, payload, offs, table_ids, segments, lanes,
                     (long long)elems_per_image, eseg, T, values, bad_streams);
}

extern "C" int sntc_scale_table_ids(const float* hyper, int64_t npix, int c, uint16_t* table_ids, void* stream) {
  if (!hyper || !table_ids || npix < 1 || c < 1) return fail(SNTC_ERR_BAD_SHAPE, "sntc_scale_table_ids: bad argument");
  hipLaunchKernelGGL(scale_index_kernel, dim3(blocks_for(npix * c)), dim3(256), 0, (hipStream_t)stream, hyper, (long long)npix, c, table_ids);
  SNTC_HIP(hipGetLastError());
  return SNTC_OK;
}

extern "C" int sntc_channel_table_ids(int64_t npix, int c, uint16_t* table_ids, void* stream) {
  if (!table_ids || npix < 1 || c < 1) return fail(SNTC_ERR_BAD_SHAPE, "sntc_channel_table_ids: bad argument");
  hipLaunchKernelGGL(channel_index_kernel, dim3(blocks_for(npix * c)), dim3(256), 0, (hipStream_t)stream, (long long)npix, c, table_ids);
  SNTC_HIP(hipGetLastError());
  return SNTC_OK;
}

extern "C" int sntc_round_to_int(const float* x, int64_t total, int32_t* out, void* stream) {
  if (!x || !out || total < 1) return fail(SNTC_ERR_BAD_SHAPE, "sntc_round_to_int: bad argument");
  hipLaunchKernelGGL(round_to_int_kernel, dim3(blocks_for(total)), dim3(256), 0, (hipStream_t)stream, x, (long long)total, out);
  SNTC_HIP(hipGetLastError());
  return SNTC_OK;
}

extern "C" int sntc_int_to_float(const int32_t* x, int64_t total, float* out, void* stream) {
  if (!x || !out || total < 1) return fail(SNTC_ERR_BAD_SHAPE, "sntc_int_to_float: bad argument");
  hipLaunchKernelGGL(int_to_float_kernel, dim3(blocks_for(total)), dim3(256), 0, (hipStream_t)stream, x, (long long)total, out);
  SNTC_HIP(hipGetLastError());
  return SNTC_OK;
}
