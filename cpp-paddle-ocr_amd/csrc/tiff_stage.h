// Expanded TIFF chunks -> device pixels for a batch of images (host side of kernels_tiff.hip).
#pragma once
#include <string>
#include <vector>

#include "image_stage.h"
#include "kernels_tiff.h"

namespace ocr {

struct TiffScratch {
  DevBuf<uint8_t> data;
  DevBuf<TiffImageDesc> id;
  PinnedStage stage;  // of the expanded chunks
};
// what a batch launched, for a caller that repeats it (ocr_tiff_time): id[first[k]] .. + count[k] are the frames of kind k
struct TiffLaunch {
  int first[kTiffKinds] = {}, count[kTiffKinds] = {};
  unsigned long long units[kTiffKinds] = {};
  size_t bytes = 0;  // of the upload
};
// why a frame is refused, nullptr when it is sound: a kernel only ever sees descriptors that passed
const char* tiff_frame_fault(const ocr_tiff_frame& f);
// Validates, stages the chunks through pinned memory and enqueues upload + pixel stage on `s`; image i is written as packed
// BGR to dst[i] (device), height x width.  Returns an OCR_* code.
int tiff_decode_async(const ocr_tiff_frame* const* imgs, int count, uint8_t* const* dst, TiffScratch& sc, hipStream_t s, std::string& err,
                      TiffLaunch* launched = nullptr);
void tiff_relaunch(const TiffScratch& sc, const TiffLaunch& L, hipStream_t s);

}  // namespace ocr
