// Inflated PNG streams -> device pixels for a batch of images (host side of kernels_png.hip).
#pragma once
#include <string>
#include <vector>

#include "image_stage.h"
#include "kernels_png.h"

namespace ocr {

struct PngScratch {
  DevBuf<uint8_t> data, recon;
  DevBuf<PngImageDesc> id;
  DevBuf<PngWork> work;
  PinnedStage stage;  // of the inflated streams
};
// what a batch launched, for a caller that repeats it (ocr_png_time): work[first[k]] .. + count[k] are the segments of kind k
struct PngLaunch {
  int first[kPngKinds] = {}, count[kPngKinds] = {};
  size_t bytes = 0;  // of the upload
};
// why a frame is refused, nullptr when it is sound: a kernel only ever sees descriptors that passed
const char* png_frame_fault(const ocr_png_frame& f);
// Validates, stages the streams through pinned memory and enqueues upload + pixel stage on `s`; image i is written as
// packed BGR to dst[i] (device), height x width.  Returns an OCR_* code.
int png_decode_async(const ocr_png_frame* const* imgs, int count, uint8_t* const* dst, PngScratch& sc, hipStream_t s, std::string& err,
                     PngLaunch* launched = nullptr);
void png_relaunch(const PngScratch& sc, const PngLaunch& L, hipStream_t s);

}  // namespace ocr
