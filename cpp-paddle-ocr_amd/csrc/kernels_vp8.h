// Host-visible launch interface of kernels_vp8.hip: the pixel half of the lossy WebP (VP8 key frame) decoder - inverse
// transforms, intra prediction, loop filter, fancy upsampling and BGR conversion, to the pixels cv::imdecode(IMREAD_COLOR) gets
// from libwebp.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../host/vp8_decode.h"  // vp8::Mb and the pixel arithmetic, stated once for host and device

namespace ocr {

constexpr int kVp8Waves = 8;     // waves of a reconstruction / filter workgroup: macroblocks of one diagonal in flight
constexpr int kVp8Block = 256;   // threads of a conversion workgroup
constexpr int kVp8Group = 4;     // output pixels of a conversion lane: 12 bytes, three dwords
constexpr int kVp8MaxGrid = 1 << 10;  // conversion workgroups per image; the units beyond are walked with a grid stride

struct Vp8ImageDesc {
  const PaddleOCR::vp8::Mb* mbs;  // device: mb_w * mb_h records
  const int16_t* coeffs;          // device
  uint8_t *y, *u, *v;             // device: planes of 16 mb_w x 16 mb_h and twice 8 mb_w x 8 mb_h, 16-byte aligned
  uint8_t* bgr;                   // device: packed BGR out, height x width, any alignment
  int width, height, mb_w, mb_h, filter_type;
  unsigned units;                 // of the conversion: one group of pixels each (kernels_vp8.hip)
};

// The three kernels over imgs[0 .. nimg), in order: reconstruction, loop filter (skipped when no frame has one: any_filter),
// conversion.  max_units: the largest Vp8ImageDesc::units.
void launch_vp8(const Vp8ImageDesc* imgs, int nimg, bool any_filter, unsigned max_units, hipStream_t s);

}  // namespace ocr
