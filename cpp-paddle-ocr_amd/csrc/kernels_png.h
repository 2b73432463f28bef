// Host-visible launch interface of kernels_png.hip: the pixel half of the PNG decoder (unfilter, conversion to packed
// BGR as cv::imdecode(IMREAD_COLOR) gives it, Adam7 placement).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ocr {

struct PngPassDesc {   // host/png_decode.h Pass
  size_t offset;       // of the pass's first filter byte in the inflated stream
  int rows, cols;
  int rowbytes;        // without the filter byte
  int x0, y0, dx, dy;
};
struct PngImageDesc {
  const uint8_t* data; // device: the inflated stream (filter byte + filtered bytes per scanline, pass after pass)
  uint8_t* recon;      // device: as large as data; holds the reconstructed LAST row of every band that another band follows
  uint8_t* bgr;        // device: packed BGR out, height x width
  int width, height, depth, ctype;
  PngPassDesc pass[7];
  uint8_t palette[768];
};
struct PngWork { int img, pass, first_row, rows; };  // one segment: rows [first_row, first_row + rows) of a pass of imgs[img]

// one kernel instantiation per filter distance (bytes per pixel, 1 for the sub-byte depths): the byte chains of a pixel
// live in registers
constexpr int kPngKinds = 6;
constexpr int kPngBpp[kPngKinds] = {1, 2, 3, 4, 6, 8};
inline int png_kind(int bpp) { for (int k = 0; k < kPngKinds; ++k) if (kPngBpp[k] == bpp) return k; return -1; }
constexpr int kPngMaxSegments = 1 << 16, kPngMaxRows = 1 << 14;  // per image / per pass: host/png_decode.h kMaxSegments, kMaxDeviceRows
constexpr int kPngBand = 64;   // rows of a band = lanes of a wave
constexpr int kPngTile = 64;   // filter units (pixels; bytes for the sub-byte depths) per row that one LDS flush writes
// One launch: work[0 .. nwork) are segments of images of one kind; a workgroup (one wave) per segment.
void launch_png(int kind, const PngImageDesc* imgs, const PngWork* work, int nwork, hipStream_t s);

}  // namespace ocr
