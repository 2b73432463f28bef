// Host-visible launch interface of kernels_tiff_fax.hip: the expansion of a TIFF's CCITT fax chunks (Compression 2, 32771, 3
// and 4) to the bytes tiff::unfax_all (host/tiff_decode.h, host/ccitt_decode.h) gives, each chunk at its nominal size in the
// buffer the pixel stage reads.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "tiff_desc.h"  // TiffFaxDesc, kTiffFaxMaxWidth, kTiffFaxList

namespace ocr {

constexpr int kTiffFaxWave = 64;         // a chunk belongs to one wavefront, and a workgroup is one wavefront
constexpr int kTiffFaxWindow = 1024;     // coded bytes staged in LDS at a time

// One workgroup a chunk, in the order of the list.  Reads pool[src .. src + byte_len) and writes out[dst .. dst + nominal) per
// chunk and nothing else, whatever the bytes and the fields are.
void launch_tiff_fax(const TiffFaxDesc* chunks, uint32_t count, const uint8_t* pool, uint8_t* out, hipStream_t s);

}  // namespace ocr
