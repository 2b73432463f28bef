// Host-visible launch interface of kernels_tiff.hip: the pixel half of the TIFF decoder (horizontal-differencing predictor,
// tile placement, planar to chunky, bit expansion, palette, MinIsWhite, 16 -> 8 bits, CMYK, alpha -> packed BGR as
// cv::imdecode(IMREAD_COLOR) gives it through libtiff's RGBA interface).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "tiff_desc.h"  // TiffImageDesc, TiffMode, kTiffKinds, kTiffRun, tiff_lanes_per_row

namespace ocr {

constexpr int kTiffBlock = 256;        // threads of a workgroup: four waves, each on units of its own
constexpr int kTiffWaves = kTiffBlock / 64;
constexpr int kTiffMaxGrid = 1 << 11;  // workgroups of a launch; the units beyond are walked with a grid stride

// One launch: imgs[0 .. nimg) are frames of one kind, total_units = the sum of their units.
void launch_tiff(int kind, const TiffImageDesc* imgs, int nimg, unsigned long long total_units, hipStream_t s);

// A plain device copy of the first bytes / 16 * 16 bytes (dst and src 16-aligned): what the pixel stage's time is set against.
void launch_plain_copy(void* dst, const void* src, size_t bytes, hipStream_t s);

}  // namespace ocr
