// Entropy-decoded lossless WebP frames -> device pixels for a batch of images (host side of kernels_webp.hip).
#pragma once
#include <string>
#include <vector>

#include "image_stage.h"
#include "kernels_webp.h"

namespace ocr {

struct WebpScratch {
  DevBuf<uint8_t> data;     // the coded images and sub-images of a batch
  DevBuf<uint32_t> recon;   // the replayed rows
  DevBuf<WebpImageDesc> id;
  PinnedStage stage;
};
// what a batch launched, for a caller that repeats it (ocr_webp_time): id[first[k]] .. + count[k] are the frames of kind k
struct WebpLaunch {
  int first[kWebpKinds] = {}, count[kWebpKinds] = {};
  unsigned long long units = 0;  // of the streaming launch
  size_t bytes = 0;              // of the upload
};
// why a frame is refused, nullptr when it is sound: a kernel only ever sees descriptors that passed
const char* webp_frame_fault(const ocr_webp_frame& f);
// Validates, stages the coded data through pinned memory and enqueues upload + pixel stage on `s`; image i is written as packed
// BGR to dst[i] (device), height x width.  Returns an OCR_* code.
int webp_decode_async(const ocr_webp_frame* const* imgs, int count, uint8_t* const* dst, WebpScratch& sc, hipStream_t s, std::string& err,
                      WebpLaunch* launched = nullptr);
void webp_relaunch(const WebpScratch& sc, const WebpLaunch& L, hipStream_t s);

}  // namespace ocr
