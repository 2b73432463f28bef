// Expanded TIFF chunks -> device pixels for a batch of images (host side of kernels_tiff.hip).
#pragma once
#include <string>
#include <vector>

#include "image_stage.h"
#include "kernels_tiff.h"
#include "kernels_inflate.h"
#include "kernels_tiff_fax.h"
#include "kernels_tiff_lzw.h"

namespace ocr {

struct TiffScratch {
  DevBuf<uint8_t> data;
  DevBuf<TiffImageDesc> id;
  PinnedStage stage;  // of the expanded chunks; a coded batch: of its chunk records and their bytes
  DevBuf<uint8_t> coded;  // a coded batch: the chunk records, then the byte pool (data is then filled by the expansion)
  DevBuf<uint32_t> produced;  // a Deflate batch: the bytes each chunk's stream gave, in the order of the records
  PinnedStage counts;  // the same on the host, pinned: the read-back is then a plain asynchronous copy
  const uint32_t* produced_host() const { return (const uint32_t*)counts.p; }
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
  // a Deflate batch: the streams the inflate launch goes over (device), instead of chunks / lzw / runs
  const InflateDesc* streams = nullptr;
  uint32_t nstreams = 0;
  // a fax batch: the chunks the fax expansion goes over (device), instead of either
  const TiffFaxDesc* fax = nullptr;
  uint32_t nfax = 0;
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
// Deflate frames (ocr_tiff_coded with compression 8 or 32946).  tiff_deflate_fault checks the frame and the chunk records - the
// rules of a coded frame with that compression set and the same device bounds - and looks at no stream: the inflate kernel gives
// a verdict per chunk.  tiff_deflate_decode_async, all on `s`: uploads the records and the pool, runs the inflate launch into
// sc.data, copies the per-chunk counts back and WAITS for that copy (4 bytes a chunk: the one host round trip of this route),
// and launches the pixel kernels only where every chunk gave the bytes its rows need; otherwise OCR_ERR_ARG "deflate: a
// chunk's stream does not hold the bytes its rows need (frame F, chunk C)" - F is ids[i] where ids is given, else i - and no
// pixel kernel is launched for the batch.  `pixels` false: the inflate launch and the read-back alone, no refusal; produced:
// count pointers (or null), each to chunks_len words in the frame's chunk order.
const char* tiff_deflate_fault(const ocr_tiff_coded& c);
int tiff_deflate_decode_async(const ocr_tiff_coded* const* imgs, int count, uint8_t* const* dst, TiffScratch& sc, hipStream_t s, std::string& err,
                              TiffLaunch* launched = nullptr, bool pixels = true, uint32_t* const* produced = nullptr, const int* ids = nullptr);
// Fax frames (ocr_tiff_fax: Compression 2, 3, 4, 32771).  tiff_fax_fault: the frame, what the coding asks of it, the records,
// the walk of every stream (tiff::fax_fault_of), the device bounds and the widest chunk (kTiffFaxMaxWidth).
// tiff_fax_decode_async as tiff_coded_decode_async, with the fax expansion (tiff_fax_relaunch) in the expansion's place.
const char* tiff_fax_fault(const ocr_tiff_fax& c);
int tiff_fax_decode_async(const ocr_tiff_fax* const* imgs, int count, uint8_t* const* dst, TiffScratch& sc, hipStream_t s, std::string& err,
                          TiffLaunch* launched = nullptr, bool pixels = true);
void tiff_fax_relaunch(const TiffScratch& sc, const TiffLaunch& L, hipStream_t s);
// the inflate launch and its read-back again (ocr_tiff_time_deflate)
int tiff_inflate_relaunch(TiffScratch& sc, const TiffLaunch& L, hipStream_t s);  // (after a tiff_deflate_decode_async of the batch)

}  // namespace ocr
