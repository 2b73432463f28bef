// JPEG 2000 frame descriptors -> device pixels for a batch of images (host side of kernels_j2k.hip).
#pragma once
#include <string>
#include <vector>

#include "image_stage.h"
#include "kernels_j2k.h"

namespace ocr {

struct J2kScratch {
  DevBuf<uint8_t> data;          // a batch's coefficients (plane a), then steps, tile-components, tiles and units
  DevBuf<int32_t> rows, recon;   // planes b and r
  PinnedStage stage;
};
// what a batch launched, for a caller that repeats it (ocr_j2k_time)
struct J2kLaunch {
  J2kBatch batch{};
  std::vector<J2kStep> steps;
  uint32_t fin_first = 0, fin_count = 0;
  size_t bytes = 0;  // of the upload
};
// why a frame is refused, nullptr when it is sound: a kernel only ever sees descriptors that passed
const char* j2k_frame_fault(const ocr_j2k_frame& f);
// Validates, stages the descriptors through pinned memory and enqueues upload + the kernels on `s`; image i is written as
// packed BGR to dst[i] (device), height x width.  Returns an OCR_* code.
int j2k_decode_async(const ocr_j2k_frame* const* imgs, int count, uint8_t* const* dst, J2kScratch& sc, hipStream_t s, std::string& err,
                     J2kLaunch* launched = nullptr);
void j2k_relaunch(const J2kLaunch& L, hipStream_t s);

}  // namespace ocr
