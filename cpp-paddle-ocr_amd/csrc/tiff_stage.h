// Expanded TIFF chunks -> device pixels for a batch of images (host side of kernels_tiff.hip).
#pragma once
#include <string>
#include <vector>

#include "image_stage.h"
#include "kernels_tiff.h"
#include "kernels_tiff_lzw.h"

namespace ocr {

struct TiffScratch {
  DevBuf<uint8_t> data;
  DevBuf<TiffImageDesc> id;
  PinnedStage stage;  // of the expanded chunks; a coded batch: of its chunk records and their bytes
  DevBuf<uint8_t> coded;  // a coded batch: the chunk records, then the byte pool (data is then filled by the expansion)
};
// what a batch launched, for a caller that repeats it (ocr_tiff_time): id[first[k]] .. + count[k] are the frames of kind k
struct TiffLaunch {
  int first[kTiffKinds] = {}, count[kTiffKinds] = {};
  unsigned long long units[kTiffKinds] = {};
  size_t bytes = 0;  // of the upload
  // a coded batch: what the expansion launches over (device)
  const TiffChunkDesc* chunks = nullptr;
  uint32_t lzw = 0, runs = 0;
  const uint8_t* pool = nullptr;
};
// why a frame is refused, nullptr when it is sound: a kernel only ever sees descriptors that passed
const char* tiff_frame_fault(const ocr_tiff_frame& f);
// Validates, stages the chunks through pinned memory and enqueues upload + pixel stage on `s`; image i is written as packed
// BGR to dst[i] (device), height x width.  Returns an OCR_* code.
int tiff_decode_async(const ocr_tiff_frame* const* imgs, int count, uint8_t* const* dst, TiffScratch& sc, hipStream_t s, std::string& err,
                      TiffLaunch* launched = nullptr);
void tiff_relaunch(const TiffScratch& sc, const TiffLaunch& L, hipStream_t s);
// The same for coded frames (ocr_tiff_coded): chunk records and bytes are uploaded, the expansion fills the chunks in device
// scratch (tiff_expand_relaunch), then the pixel kernels run (tiff_relaunch) - all on `s`.  `pixels` false: the expansion
// alone, dst unused; frame i's chunks then lie in sc.data in the order of the batch, each frame padded to 256 bytes.
const char* tiff_coded_fault(const ocr_tiff_coded& c);
int tiff_coded_decode_async(const ocr_tiff_coded* const* imgs, int count, uint8_t* const* dst, TiffScratch& sc, hipStream_t s, std::string& err,
                            TiffLaunch* launched = nullptr, bool pixels = true);
void tiff_expand_relaunch(const TiffScratch& sc, const TiffLaunch& L, hipStream_t s);

}  // namespace ocr
