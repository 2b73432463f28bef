// Host-visible launch interface of kernels_raw.hip: the pixel half of the BMP / PNM decoders (bit, nibble and palette
// expansion, 5-5-5 / 5-6-5, high bytes of 16-bit samples, row order, channel order -> packed BGR as
// cv::imdecode(IMREAD_COLOR) gives it).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ocr {

constexpr int kRawKinds = 12;          // ocr_raw_kind
constexpr int kRawBlock = 256;         // threads of a workgroup
constexpr int kRawGroup = 4;           // pixels of a lane: 12 output bytes, three whole dwords
constexpr int kRawMaxGrid = 1 << 13;   // workgroups of a launch; the units beyond are walked with a grid stride

// A unit of work = a span of one output row: kRawBlock groups of kRawGroup pixels (span 0 also takes the row's head, the
// up to three pixels in front of the first 4-aligned output address).  A frame has height * spans units, numbered row by
// row from first_unit; the units of the frames of one launch are consecutive.
struct RawImageDesc {
  const uint8_t* data;      // device: the stored rows, 4-aligned (the staging packs frames at multiples of 256)
  uint8_t* bgr;             // device: packed BGR out, height x width, any alignment
  unsigned long long first_unit;
  size_t row_stride;
  int width, height, bottom_up;
  unsigned spans;           // units per row (>= 1)
  uint32_t palette[256];    // B | G << 8 | R << 16
};

// spans of a row of `width` pixels: whatever the head is (0 .. 3 pixels), the groups behind it number at most this many
inline unsigned raw_spans(int width) { return (unsigned)(((size_t)width + kRawGroup - 1) / kRawGroup + kRawBlock - 1) / kRawBlock; }

// One launch: imgs[0 .. nimg) are frames of one kind, total_units = the sum of their units.
void launch_raw(int kind, const RawImageDesc* imgs, int nimg, unsigned long long total_units, hipStream_t s);

}  // namespace ocr
