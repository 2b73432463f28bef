// What the TIFF kernels are handed, with nothing of HIP in it: the image descriptor of the pixel stage (kernels_tiff.hip) and
// the per-chunk records of the three expansions (kernels_tiff_lzw.hip, kernels_inflate.hip, kernels_tiff_fax.hip).  The host
// fills them in tiff_plan.h, which a plain host program can run; the kernels_*.h headers declare the launches over them.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace ocr {

constexpr int kTiffKinds = 3;  // by sample width: below 8 bits, 8 bits, 16 bits - one launch each
constexpr int kTiffRun = 4;    // pixels of a lane: its run of the scan, and 12 output bytes

enum TiffMode { TIFF_GREY, TIFF_PALETTE, TIFF_RGB, TIFF_GREY_PLANES, TIFF_CMYK };

// A unit of work = what ONE WAVE does: rows_per_unit rows of one chunk (several when the chunk's rows are narrow:
// lanes_per_row = the power of two that covers a row in runs of kTiffRun, at most 64), each walked span by span with the
// scan's carry in a register.  A frame has chunks * units_per_chunk units, chunk by chunk from first_unit; the units of the
// frames of one launch are consecutive.
struct TiffImageDesc {
  const uint8_t* data;      // device: the expanded chunks at their nominal size
  uint8_t* bgr;             // device: packed BGR out, height x width, any alignment
  unsigned long long first_unit;
  size_t chunk_bytes, plane_bytes;  // plane_bytes: between the planes of planar 2 (0 when chunky)
  size_t row_bytes;                 // of a chunk's row
  int width, height, tile_width, tile_height, across, down;
  int bits, samples, used, mode;
  int predictor, big_endian, invert, premultiply;
  int lanes_per_row, rows_per_unit;
  unsigned units_per_chunk;
  uint32_t palette[256];    // B | G << 8 | R << 16
};

inline int tiff_lanes_per_row(int tile_width) {
  const int runs = (tile_width + kTiffRun - 1) / kTiffRun;
  int l = 1;
  while (l < 64 && l < runs) l <<= 1;
  return l;
}

struct TiffChunkDesc {  // a chunk of the batch; the host's extent scan (tiff::coded_fault) has passed its stream
  uint64_t src;         // into the batch's byte pool
  uint64_t dst;         // into the batch's expanded chunks
  uint32_t byte_len;    // coded bytes
  uint32_t need;        // rows * row bytes: what the stream expands to
  uint32_t nominal;     // tile_height * row bytes >= need: what is written, zeros behind `need`
  uint32_t compression; // 1, 5 or 32773
};

struct InflateDesc {   // a stream of the batch; nobody has looked at its bytes
  uint64_t src;        // into the batch's byte pool
  uint64_t dst;        // into the batch's output
  uint32_t byte_len;   // coded bytes
  uint32_t need;       // the bytes the stream must give: what is asked of it, and no more is written
  uint32_t nominal;    // >= need: what is written, zeros behind what the stream gave
};

constexpr int kTiffFaxMaxWidth = 8192;              // pixels of a chunk's row: what the two lists of changing elements have room for
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

}  // namespace ocr
