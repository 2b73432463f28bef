// Host-visible launch interface of kernels_tiff.hip: the pixel half of the TIFF decoder (horizontal-differencing predictor,
// tile placement, planar to chunky, bit expansion, palette, MinIsWhite, 16 -> 8 bits, CMYK, alpha -> packed BGR as
// cv::imdecode(IMREAD_COLOR) gives it through libtiff's RGBA interface).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ocr {

constexpr int kTiffKinds = 3;          // by sample width: below 8 bits, 8 bits, 16 bits - one launch each
constexpr int kTiffBlock = 256;        // threads of a workgroup: four waves, each on units of its own
constexpr int kTiffWaves = kTiffBlock / 64;
constexpr int kTiffRun = 4;            // pixels of a lane: its run of the scan, and 12 output bytes
constexpr int kTiffMaxGrid = 1 << 11;  // workgroups of a launch; the units beyond are walked with a grid stride

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

// One launch: imgs[0 .. nimg) are frames of one kind, total_units = the sum of their units.
void launch_tiff(int kind, const TiffImageDesc* imgs, int nimg, unsigned long long total_units, hipStream_t s);

// A plain device copy of the first bytes / 16 * 16 bytes (dst and src 16-aligned): what the pixel stage's time is set against.
void launch_plain_copy(void* dst, const void* src, size_t bytes, hipStream_t s);

}  // namespace ocr
