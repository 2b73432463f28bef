// The frame kinds a pipeline stages (ocr_frame_kind): one row per kind with what the staging path asks of it.  A new
// kind is an enum value, a row here and a scratch member below; pipe.hip names no kind.
#pragma once
#include <cstddef>

#include "j2k_stage.h"
#include "jpeg_stage.h"
#include "png_stage.h"
#include "raw_stage.h"
#include "tiff_stage.h"
#include "vp8_stage.h"
#include "webp_stage.h"

namespace ocr {

// A pipeline's scratch, one per kind: the frames of a kind in a batch are one *_decode_async call, and kinds whose
// descriptor type is the same (expanded, coded and Deflate TIFF; JPEG 2000 coefficients and coded blocks) are still
// separate calls, because their uploads differ.
struct FrameScratch {
  JpegScratch jpeg;
  PngScratch png;
  RawScratch raw;
  TiffScratch tiff, tiff_coded, tiff_deflate, tiff_fax;
  WebpScratch webp;
  Vp8Scratch vp8;
  J2kScratch j2k, j2k_coded;
};

struct FrameKind {
  // why a frame is refused, nullptr when it is sound
  const char* (*fault)(const void* frame);
  // the size of the decoded image (of a sound frame)
  void (*size)(const void* frame, int& rows, int& cols);
  // the kind's *_decode_async on `s`; ids[i]: frame i's place in the caller's batch, for a refusal that names a frame
  int (*decode)(const void* const* frames, int count, uint8_t* const* dst, FrameScratch& sc, hipStream_t s, std::string& err, const int* ids);
};

namespace frame_kinds {  // (internal linkage: the table is their one user)

template <class F, const char* (*Fault)(const F&)>
static const char* fault(const void* frame) { return Fault(*(const F*)frame); }

// F: the descriptor, or the ocr_tiff_frame / ocr_j2k_frame that a coded descriptor starts with (its `frame` member)
template <class F>
static void size(const void* frame, int& rows, int& cols) { rows = ((const F*)frame)->height; cols = ((const F*)frame)->width; }
// the oriented size: a 40 x 72 image and a 72 x 40 one that EXIF turns by 90 degrees share a size group and a det pass
inline void jpeg_size(const void* frame, int& rows, int& cols) {
  rows = jpeg_out_rows(*(const ocr_jpeg_frame*)frame);
  cols = jpeg_out_cols(*(const ocr_jpeg_frame*)frame);
}
static_assert(offsetof(ocr_tiff_coded, frame) == 0 && offsetof(ocr_j2k_coded, frame) == 0, "a coded descriptor starts with its frame");
static_assert(offsetof(ocr_tiff_fax, coded) == 0, "a fax descriptor starts with its coded frame, and that with its frame");

template <class F, class S, class L, int (*Decode)(const F* const*, int, uint8_t* const*, S&, hipStream_t, std::string&, L*), S FrameScratch::*Sc>
static int decode(const void* const* frames, int count, uint8_t* const* dst, FrameScratch& sc, hipStream_t s, std::string& err, const int*) {
  return Decode((const F* const*)frames, count, dst, sc.*Sc, s, err, nullptr);
}
inline int j2k_coded_decode(const void* const* frames, int count, uint8_t* const* dst, FrameScratch& sc, hipStream_t s, std::string& err, const int*) {
  return j2k_coded_decode_async((const ocr_j2k_coded* const*)frames, count, dst, sc.j2k_coded, s, err);
}
// the coded TIFF routes: one staging function over the route; ids reach the one route that names a frame in a refusal (Deflate)
template <TiffRouteKind R>
static const char* tiff_route_fault(const void* frame) { return tiff_coded_fault(R, *(const ocr_tiff_coded*)frame); }
template <TiffRouteKind R, TiffScratch FrameScratch::*Sc>
static int tiff_route_decode(const void* const* frames, int count, uint8_t* const* dst, FrameScratch& sc, hipStream_t s, std::string& err, const int* ids) {
  return tiff_coded_decode_async(R, (const ocr_tiff_coded* const*)frames, count, dst, sc.*Sc, s, err, nullptr, true, nullptr, ids);
}

}  // namespace frame_kinds

// indexed by ocr_frame_kind
inline const FrameKind kFrameKinds[] = {
    /* JPEG */ {frame_kinds::fault<ocr_jpeg_frame, jpeg_frame_fault>, frame_kinds::jpeg_size,
                frame_kinds::decode<ocr_jpeg_frame, JpegScratch, JpegLaunch, jpeg_decode_async, &FrameScratch::jpeg>},
    /* PNG */ {frame_kinds::fault<ocr_png_frame, png_frame_fault>, frame_kinds::size<ocr_png_frame>,
               frame_kinds::decode<ocr_png_frame, PngScratch, PngLaunch, png_decode_async, &FrameScratch::png>},
    /* RAW */ {frame_kinds::fault<ocr_raw_frame, raw_frame_fault>, frame_kinds::size<ocr_raw_frame>,
               frame_kinds::decode<ocr_raw_frame, RawScratch, RawLaunch, raw_decode_async, &FrameScratch::raw>},
    /* TIFF */ {frame_kinds::fault<ocr_tiff_frame, tiff_frame_fault>, frame_kinds::size<ocr_tiff_frame>,
                frame_kinds::decode<ocr_tiff_frame, TiffScratch, TiffLaunch, tiff_decode_async, &FrameScratch::tiff>},
    /* WEBP */ {frame_kinds::fault<ocr_webp_frame, webp_frame_fault>, frame_kinds::size<ocr_webp_frame>,
                frame_kinds::decode<ocr_webp_frame, WebpScratch, WebpLaunch, webp_decode_async, &FrameScratch::webp>},
    /* VP8 */ {frame_kinds::fault<ocr_vp8_frame, vp8_frame_fault>, frame_kinds::size<ocr_vp8_frame>,
               frame_kinds::decode<ocr_vp8_frame, Vp8Scratch, Vp8Launch, vp8_decode_async, &FrameScratch::vp8>},
    /* J2K */ {frame_kinds::fault<ocr_j2k_frame, j2k_frame_fault>, frame_kinds::size<ocr_j2k_frame>,
               frame_kinds::decode<ocr_j2k_frame, J2kScratch, J2kLaunch, j2k_decode_async, &FrameScratch::j2k>},
    /* J2K_CODED */ {frame_kinds::fault<ocr_j2k_coded, j2k_coded_fault>, frame_kinds::size<ocr_j2k_frame>, frame_kinds::j2k_coded_decode},
    /* TIFF_CODED */ {frame_kinds::tiff_route_fault<tiff_plan::kCoded>, frame_kinds::size<ocr_tiff_frame>,
                      frame_kinds::tiff_route_decode<tiff_plan::kCoded, &FrameScratch::tiff_coded>},
    /* TIFF_DEFLATE */ {frame_kinds::tiff_route_fault<tiff_plan::kDeflate>, frame_kinds::size<ocr_tiff_frame>,
                        frame_kinds::tiff_route_decode<tiff_plan::kDeflate, &FrameScratch::tiff_deflate>},
    /* TIFF_FAX */ {frame_kinds::tiff_route_fault<tiff_plan::kFax>, frame_kinds::size<ocr_tiff_frame>,
                    frame_kinds::tiff_route_decode<tiff_plan::kFax, &FrameScratch::tiff_fax>},
};
constexpr int kFrameKindCount = (int)(sizeof kFrameKinds / sizeof kFrameKinds[0]);
static_assert(kFrameKindCount == OCR_FRAME_TIFF_FAX + 1 && OCR_FRAME_TIFF_DEFLATE == 9 && OCR_FRAME_JPEG == 0 && OCR_FRAME_PNG == 1 && OCR_FRAME_RAW == 2 && OCR_FRAME_TIFF == 3 &&
                  OCR_FRAME_WEBP == 4 && OCR_FRAME_VP8 == 5 && OCR_FRAME_J2K == 6 && OCR_FRAME_J2K_CODED == 7 && OCR_FRAME_TIFF_CODED == 8,
              "kFrameKinds is in the order of ocr_frame_kind");

// The order in which a batch's kinds are enqueued on the copy stream.  Deflate TIFF first: it is the one route that can
// refuse a stream (it waits for its inflate verdicts), and it does so before anything else is enqueued; the others in
// the order of the enum.
constexpr int kFrameLaunchOrder[kFrameKindCount] = {OCR_FRAME_TIFF_DEFLATE, OCR_FRAME_JPEG, OCR_FRAME_PNG, OCR_FRAME_RAW,       OCR_FRAME_TIFF,
                                                    OCR_FRAME_WEBP,         OCR_FRAME_VP8,  OCR_FRAME_J2K, OCR_FRAME_J2K_CODED, OCR_FRAME_TIFF_CODED,
                                                    OCR_FRAME_TIFF_FAX};

}  // namespace ocr
