// JPEG 2000 frame descriptors -> device pixels for a batch of images (host side of kernels_j2k.hip).
#pragma once
#include <string>
#include <vector>

#include "image_stage.h"
#include "kernels_j2k.h"
#include "kernels_j2k_t1.h"

namespace ocr {

struct J2kScratch {
  DevBuf<uint8_t> data;          // a batch's coefficients (plane a), then steps, tile-components, tiles and units; a coded
                                 // batch: then its blocks and their bytes
  DevBuf<int32_t> rows, recon;   // planes b and r
  PinnedStage stage;
};
// what a batch launched, for a caller that repeats it (ocr_j2k_time)
struct J2kLaunch {
  J2kBatch batch{};
  std::vector<J2kStep> steps;
  uint32_t fin_first = 0, fin_count = 0;
  size_t bytes = 0;  // of the upload
  // a coded batch: plane a is not uploaded but zeroed and filled by tier-1; the upload is what follows it
  size_t plane_bytes = 0, upload_at = 0;
  const J2kT1Block* blocks = nullptr;  // device
  uint32_t nblocks = 0;
  const uint8_t* pool = nullptr;       // device
};
// why a frame is refused, nullptr when it is sound: a kernel only ever sees descriptors that passed
const char* j2k_frame_fault(const ocr_j2k_frame& f);
// Validates, stages the descriptors through pinned memory and enqueues upload + the kernels on `s`; image i is written as
// packed BGR to dst[i] (device), height x width.  Returns an OCR_* code.
int j2k_decode_async(const ocr_j2k_frame* const* imgs, int count, uint8_t* const* dst, J2kScratch& sc, hipStream_t s, std::string& err,
                     J2kLaunch* launched = nullptr);
void j2k_relaunch(const J2kLaunch& L, hipStream_t s);
// The same for coded frames (ocr_j2k_coded): blocks, bytes and descriptors are uploaded, plane a is zeroed and filled by
// tier-1 (j2k_t1_relaunch), then the pixel kernels run (j2k_relaunch) - all on `s`.  `pixels` false: tier-1 alone, dst unused.
const char* j2k_coded_fault(const ocr_j2k_coded& c);
int j2k_coded_decode_async(const ocr_j2k_coded* const* imgs, int count, uint8_t* const* dst, J2kScratch& sc, hipStream_t s, std::string& err,
                           J2kLaunch* launched = nullptr, bool pixels = true);
hipError_t j2k_t1_relaunch(const J2kLaunch& L, hipStream_t s);

}  // namespace ocr
