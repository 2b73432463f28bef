// Stored BMP / PNM rows -> device pixels for a batch of images (host side of kernels_raw.hip).
#pragma once
#include <string>
#include <vector>

#include "image_stage.h"
#include "kernels_raw.h"

namespace ocr {

struct RawScratch {
  DevBuf<uint8_t> data;
  DevBuf<RawImageDesc> id;
  PinnedStage stage;  // of the stored rows
};
// what a batch launched, for a caller that repeats it (ocr_raw_time): id[first[k]] .. + count[k] are the frames of kind k
struct RawLaunch {
  int first[kRawKinds] = {}, count[kRawKinds] = {};
  unsigned long long units[kRawKinds] = {};
  size_t bytes = 0;  // of the upload
};
// why a frame is refused, nullptr when it is sound: a kernel only ever sees descriptors that passed
const char* raw_frame_fault(const ocr_raw_frame& f);
// Validates, stages the rows through pinned memory and enqueues upload + pixel stage on `s`; image i is written as packed
// BGR to dst[i] (device), height x width.  Returns an OCR_* code.
int raw_decode_async(const ocr_raw_frame* const* imgs, int count, uint8_t* const* dst, RawScratch& sc, hipStream_t s, std::string& err,
                     RawLaunch* launched = nullptr);
void raw_relaunch(const RawScratch& sc, const RawLaunch& L, hipStream_t s);

}  // namespace ocr
