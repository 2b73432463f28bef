// JPEG coefficients -> device pixels for a batch of images (host side of kernels_jpeg.hip).
#pragma once
#include <string>
#include <vector>

#include "image_stage.h"
#include "kernels_jpeg.h"

namespace ocr {

struct JpegScratch {
  DevBuf<int16_t> coef;
  DevBuf<uint8_t> planes;
  DevBuf<JpegPlaneDesc> pd;
  DevBuf<JpegImageDesc> id;
  DevBuf<JpegGenDesc> gd;
  PinnedStage stage;  // of the coefficients
};
// Validates the descriptors, stages the coefficients through pinned memory, and enqueues upload + IDCT + upsampling /
// colour conversion + EXIF orientation on `s`; image i is written as packed BGR to dst[i] (device), jpeg_out_rows x
// jpeg_out_cols.  launched: the kernels' launch parameters, for a caller that repeats them (ocr_jpeg_time).
// Returns an OCR_* code.
int jpeg_decode_async(const ocr_jpeg_frame* const* imgs, int count, uint8_t* const* dst, JpegScratch& sc, hipStream_t s, std::string& err,
                      JpegLaunch* launched = nullptr);
bool jpeg_img_valid(const ocr_jpeg_img& im);
// why a frame is refused, nullptr when it is sound
const char* jpeg_frame_fault(const ocr_jpeg_frame& f);
// the frame that says what a (valid) ocr_jpeg_img says: luma at hmax x vmax, chroma 1x1, grey or YCbCr
ocr_jpeg_frame jpeg_frame_of(const ocr_jpeg_img& im);
// the kernel an image runs in (kernels_jpeg.h): the kinds of before for what ocr_jpeg_img can hold, else a general kind
int jpeg_frame_kind(const ocr_jpeg_frame& f);
inline int jpeg_out_rows(const ocr_jpeg_frame& im) { return im.orientation >= 5 ? im.cols : im.rows; }
inline int jpeg_out_cols(const ocr_jpeg_frame& im) { return im.orientation >= 5 ? im.rows : im.cols; }

}  // namespace ocr
