// VP8 frame descriptors -> device pixels for a batch of images (host side of kernels_vp8.hip).
#pragma once
#include <string>
#include <vector>

#include "image_stage.h"
#include "kernels_vp8.h"

namespace ocr {

struct Vp8Scratch {
  DevBuf<uint8_t> data;    // the macroblock records and coefficients of a batch
  DevBuf<uint8_t> planes;  // Y, U, V of every image
  DevBuf<Vp8ImageDesc> id;
  PinnedStage stage;
};
// what a batch launched, for a caller that repeats it (ocr_vp8_time)
struct Vp8Launch {
  int count = 0;
  bool any_filter = false;
  unsigned max_units = 0;
  size_t bytes = 0;  // of the upload
};
// why a frame is refused, nullptr when it is sound: a kernel only ever sees descriptors that passed
const char* vp8_frame_fault(const ocr_vp8_frame& f);
// Validates, stages the descriptors through pinned memory and enqueues upload + the three kernels on `s`; image i is written as
// packed BGR to dst[i] (device), height x width.  Returns an OCR_* code.
int vp8_decode_async(const ocr_vp8_frame* const* imgs, int count, uint8_t* const* dst, Vp8Scratch& sc, hipStream_t s, std::string& err,
                     Vp8Launch* launched = nullptr);
void vp8_relaunch(const Vp8Scratch& sc, const Vp8Launch& L, hipStream_t s);

}  // namespace ocr
