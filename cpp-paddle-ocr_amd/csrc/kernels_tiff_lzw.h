// Host-visible launch interface of kernels_tiff_lzw.hip: the expansion of a TIFF's coded chunks (LZW, PackBits, stored) to the
// bytes tiff::expand (host/tiff_decode.h) gives, each chunk at its nominal size in the buffer the pixel stage reads.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ocr {

constexpr int kTiffLzwWave = 64;       // a chunk belongs to one wavefront, and a workgroup is one wavefront
constexpr int kTiffLzwEntries = 4096;  // of the LZW table: a position and a length each
constexpr int kTiffLzwWindow = 1024;   // coded bytes staged in LDS at a time

struct TiffChunkDesc {  // a chunk of the batch; the host's extent scan (tiff::coded_fault) has passed its stream
  uint64_t src;         // into the batch's byte pool
  uint64_t dst;         // into the batch's expanded chunks
  uint32_t byte_len;    // coded bytes
  uint32_t need;        // rows * row bytes: what the stream expands to
  uint32_t nominal;     // tile_height * row bytes >= need: what is written, zeros behind `need`
  uint32_t compression; // 1, 5 or 32773
};

// One workgroup a chunk, in the order of the list: chunks[0 .. lzw) are the LZW chunks (the kernel with the table), the `runs`
// behind them PackBits and stored ones.  Reads pool[src .. src + byte_len) and writes out[dst .. dst + nominal) per chunk and
// nothing else, whatever the bytes are.
void launch_tiff_expand(const TiffChunkDesc* chunks, uint32_t lzw, uint32_t runs, const uint8_t* pool, uint8_t* out, hipStream_t s);

}  // namespace ocr
