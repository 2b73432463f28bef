// Host-visible launch interface of kernels_tiff_fax.hip: the expansion of a TIFF's CCITT fax chunks (Compression 2, 32771, 3
// and 4) to the bytes tiff::unfax_all (host/tiff_decode.h, host/ccitt_decode.h) gives, each chunk at its nominal size in the
// buffer the pixel stage reads.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ocr {

constexpr int kTiffFaxWave = 64;         // a chunk belongs to one wavefront, and a workgroup is one wavefront
constexpr int kTiffFaxWindow = 1024;     // coded bytes staged in LDS at a time
constexpr int kTiffFaxMaxWidth = 8192;   // pixels of a chunk's row: what the two lists of changing elements have room for
constexpr int kTiffFaxList = kTiffFaxMaxWidth + 2;  // entries of a list: width + 1 at most are used

struct TiffFaxDesc {    // a chunk of the batch; the host's scan (tiff::fax_fault_of) has passed its stream
  uint64_t src;         // into the batch's byte pool
  uint64_t dst;         // into the batch's expanded chunks
  uint32_t byte_len;    // coded bytes
  uint32_t rows;        // the rows the stream holds
  uint32_t nominal;     // tile_height * row bytes >= rows * row bytes: what is written, zeros behind the rows
  uint32_t width;       // pixels of a row: 1 .. kTiffFaxMaxWidth; a row is (width + 7) / 8 bytes
  uint32_t compression; // 2, 3, 4 or 32771
  uint32_t t4_options;  // of Compression 3, else 0
};

// One workgroup a chunk, in the order of the list.  Reads pool[src .. src + byte_len) and writes out[dst .. dst + nominal) per
// chunk and nothing else, whatever the bytes and the fields are.
void launch_tiff_fax(const TiffFaxDesc* chunks, uint32_t count, const uint8_t* pool, uint8_t* out, hipStream_t s);

}  // namespace ocr
