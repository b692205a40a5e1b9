// rans_channels.hip -- the rANS coder of rans.hip for "one latent, table = channel": the latents of the factorized-prior
// model (reference factorized/models.py:101-124, whose entropy model is one deep-factorized density per channel).
//
// Same streams, word for word, as rans.hip codes for the same values with table id = channel (format: the head of rans.hip).
// What differs is where a lane's table id and value come from and go to: ChannelEnc / ChannelDec of rans_kernel.h.
#include "rans_kernel.h"

namespace sntc {

// the coder of rans_kernel.h on table = channel (ChannelEnc / ChannelDec): LDS = the tables staged in LDS, else read from global memory
template <bool LDS>
__global__ void __launch_bounds__(64) rans_encode_channels_kernel(const float* __restrict__ y, int segs, int L, int C, long long E,
                                                                  long long Eseg, RansTables T, long long cap,
                                                                  unsigned short* __restrict__ scratch, int* __restrict__ len_words,
                                                                  float* __restrict__ y_hat) {
  ChannelEnc src;
  src.y = y;
  src.y_hat = y_hat;
  src.C = C;
  rans_encode_body<LDS>(src, segs, L, E, Eseg, T, cap, scratch, len_words);
}

template <bool LDS>
__global__ void __launch_bounds__(64) rans_decode_channels_kernel(const unsigned short* __restrict__ payload,
                                                                  const long long* __restrict__ offsets, int segs, int L, int C,
                                                                  long long E, long long Eseg, RansTables T, float* __restrict__ y_hat,
                                                                  int* __restrict__ bad) {
  ChannelDec src;
  src.out = y_hat;
  src.C = C;
  rans_decode_body<CdfSearch<LDS>>(payload, offsets, src, segs, L, E, Eseg, T, bad);
}

__global__ void __launch_bounds__(64) rans_decode_channels_fast_kernel(const unsigned short* __restrict__ payload,
                                                                       const long long* __restrict__ offsets, int segs, int L, int C,
                                                                       long long E, long long Eseg, RansDecTables T,
                                                                       float* __restrict__ y_hat, int* __restrict__ bad) {
  ChannelDec src;
  src.out = y_hat;
  src.C = C;
  rans_decode_body<StartTableSearch>(payload, offsets, src, segs, L, E, Eseg, T, bad);
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
  return rans_launch(rans_encode_channels_kernel<true>, rans_encode_channels_kernel<false>, kChanStagingBytes, T, nimages * segments,
                     (hipStream_t)stream, y, segments, lanes, channels, (long long)elems_per_image,
                     rans_segment_elems(elems_per_image, segments), T, (long long)cap_words, scratch, len_words, y_hat);
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
  RansDecTables D;
  int lds;
  if (int rc = rans_dec_tables("sntc_rans_decode_channels", kChanStagingBytes, dec, lut, meta, lut_meta, channels, total_entries, lut_entries, D,
                               lds))
    return rc;
  const long long eseg = rans_segment_elems(elems_per_image, segments);
  const int ns = nimages * segments;
  hipStream_t s = (hipStream_t)stream;
  if (int zrc = zero_async(bad_streams, sizeof(int32_t), s)) return zrc;
  const long long* offs = reinterpret_cast<const long long*>(offsets);
  if (D.dec) {
    SNTC_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(rans_decode_channels_fast_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, lds));
    hipLaunchKernelGGL(rans_decode_channels_fast_kernel, dim3(ns), dim3(64), lds, s, payload, offs, segments, lanes, channels,
                       (long long)elems_per_image, eseg, D, y_hat, bad_streams);
    SNTC_HIP(hipGetLastError());
    return SNTC_OK;
  }
  const RansTables T{cdf, reinterpret_cast<const uint2*>(meta), channels, total_entries};
  return rans_launch(rans_decode_channels_kernel<true>, rans_decode_channels_kernel<false>, kChanStagingBytes, T, ns, s, payload, offs, segments,
                     lanes, channels, (long long)elems_per_image, eseg, T, y_hat, bad_streams);
}
