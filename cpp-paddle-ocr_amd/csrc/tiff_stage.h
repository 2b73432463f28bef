// Expanded TIFF chunks -> device pixels for a batch of images (host side of kernels_tiff.hip), and the coded routes in front
// of it: what is arithmetic about a batch is tiff_plan.h, the device calls around it are capi_tiff.hip.
#pragma once
#include <string>
#include <vector>

#include "image_stage.h"
#include "kernels_tiff.h"
#include "kernels_inflate.h"
#include "kernels_tiff_fax.h"
#include "kernels_tiff_lzw.h"
#include "tiff_plan.h"

namespace ocr {

using TiffRouteKind = tiff_plan::Route;  // kCoded, kDeflate, kFax

struct TiffScratch {
  DevBuf<uint8_t> data;
  DevBuf<TiffImageDesc> id;
  PinnedStage stage;  // of the expanded chunks; a coded batch: of its chunk records and their bytes
  DevBuf<uint8_t> coded;  // a coded batch: the chunk records, then the byte pool (data is then filled by the expansion)
  DevBuf<uint32_t> produced;  // a Deflate batch: the bytes each chunk's stream gave, in the order of the records
  PinnedStage counts;  // the same on the host, pinned: the read-back is then a plain asynchronous copy
  const uint32_t* produced_host() const { return (const uint32_t*)counts.p; }
};
// what a batch launched, for a caller that repeats it (ocr_tiff_time): the frames of each kind (tiff_plan::Kinds)
struct TiffLaunch : tiff_plan::Kinds {
  size_t bytes = 0;  // of the upload
  // a coded batch: what its route's expansion launches over (device) - records of the route's type, the first `lzw` of a
  // kCoded batch its LZW chunks
  TiffRouteKind route = tiff_plan::kCoded;
  const void* records = nullptr;
  uint32_t nrecords = 0, lzw = 0;
  const uint8_t* pool = nullptr;
};
// why a frame is refused, nullptr when it is sound: a kernel only ever sees descriptors that passed
const char* tiff_frame_fault(const ocr_tiff_frame& f);
// Validates, stages the chunks through pinned memory and enqueues upload + pixel stage on `s`; image i is written as packed
// BGR to dst[i] (device), height x width.  Returns an OCR_* code.
int tiff_decode_async(const ocr_tiff_frame* const* imgs, int count, uint8_t* const* dst, TiffScratch& sc, hipStream_t s, std::string& err,
                      TiffLaunch* launched = nullptr);
void tiff_relaunch(const TiffScratch& sc, const TiffLaunch& L, hipStream_t s);
// why a coded frame of `route` is refused (tiff_plan::coded_fault), nullptr when it is sound
const char* tiff_coded_fault(TiffRouteKind route, const ocr_tiff_coded& c);
// The same for the coded frames of a route (a kFax batch: each the first member of an ocr_tiff_fax): tiff_plan::coded_fault
// per frame, then chunk records and bytes are uploaded, the route's expansion fills the chunks in device scratch
// (tiff_middle_relaunch), then the pixel kernels run (tiff_relaunch) - all on `s`.  `pixels` false: the expansion alone, dst
// unused; frame i's chunks then lie in sc.data in the order of the batch, each frame padded to 256 bytes.
// kDeflate looks at no stream on the host: after the inflate launch it copies the per-chunk counts back and WAITS for that copy
// (4 bytes a chunk: the one host round trip of the coded routes), and launches the pixel kernels only where every chunk gave
// the bytes its rows need; otherwise OCR_ERR_ARG "deflate: a chunk's stream does not hold the bytes its rows need (frame F,
// chunk C)" - F is ids[i] where ids is given, else i - and no pixel kernel is launched for the batch.  `pixels` false: no
// refusal.  produced (kDeflate): count pointers (or null), each to chunks_len words in the frame's chunk order.
int tiff_coded_decode_async(TiffRouteKind route, const ocr_tiff_coded* const* imgs, int count, uint8_t* const* dst, TiffScratch& sc, hipStream_t s,
                            std::string& err, TiffLaunch* launched = nullptr, bool pixels = true, uint32_t* const* produced = nullptr,
                            const int* ids = nullptr);
// what runs between upload and pixel stage, again (after a tiff_coded_decode_async of the batch): the expansion of L.route;
// kDeflate: with the read-back of its counts, which it waits for
hipError_t tiff_middle_relaunch(TiffScratch& sc, const TiffLaunch& L, hipStream_t s);

}  // namespace ocr
