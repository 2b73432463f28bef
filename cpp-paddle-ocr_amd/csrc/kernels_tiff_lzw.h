// Host-visible launch interface of kernels_tiff_lzw.hip: the expansion of a TIFF's coded chunks (LZW, PackBits, stored) to the
// bytes tiff::expand (host/tiff_decode.h) gives, each chunk at its nominal size in the buffer the pixel stage reads.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "tiff_desc.h"  // TiffChunkDesc

namespace ocr {

constexpr int kTiffLzwWave = 64;       // a chunk belongs to one wavefront, and a workgroup is one wavefront
constexpr int kTiffLzwEntries = 4096;  // of the LZW table: a position and a length each
constexpr int kTiffLzwWindow = 1024;   // coded bytes staged in LDS at a time

// One workgroup a chunk, in the order of the list: chunks[0 .. lzw) are the LZW chunks (the kernel with the table), the `runs`
// behind them PackBits and stored ones.  Reads pool[src .. src + byte_len) and writes out[dst .. dst + nominal) per chunk and
// nothing else, whatever the bytes are.
void launch_tiff_expand(const TiffChunkDesc* chunks, uint32_t lzw, uint32_t runs, const uint8_t* pool, uint8_t* out, hipStream_t s);

}  // namespace ocr
