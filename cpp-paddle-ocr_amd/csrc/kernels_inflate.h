// Host-visible launch interface of kernels_inflate.hip: zlib streams (RFC 1950 around RFC 1951) inflated on the device, one
// stream per wavefront.  Nothing here knows what the bytes are for: a TIFF's Deflate chunks today (capi_tiff.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "tiff_desc.h"  // InflateDesc

namespace ocr {

constexpr int kInflateWave = 64;  // a stream belongs to one wavefront, and a workgroup is one wavefront

// One workgroup a stream, in the order of the list.  Reads pool[src .. src + byte_len) and writes out[dst .. dst + nominal) and
// produced[i] per stream and nothing else, whatever the bytes are.  produced[i]: the bytes that came out before the first fault,
// the end of the final block or the end of the input, cut at min(need, nominal); the stream is good where that equals `need`
// (the rule of tiff::detail::inflate, host/tiff_decode.h: the checksum behind the final block is not read).
void launch_inflate(const InflateDesc* streams, uint32_t count, const uint8_t* pool, uint8_t* out, uint32_t* produced, hipStream_t s);

}  // namespace ocr
