// Host side of the device BMP / PNM back-end + its C-ABI entry points.
#include <algorithm>
#include <cstring>

#include "capi_common.h"
#include "raw_stage.h"

namespace ocr {

namespace {

// host/raw_decode.h row_bytes(): bytes of a stored row without padding; 0 = no such kind
size_t raw_row_bytes(int kind, size_t width) {
  switch (kind) {
    case OCR_RAW_INDEX1: case OCR_RAW_BIT1_INV: return (width + 7) / 8;
    case OCR_RAW_INDEX4: return (width + 1) / 2;
    case OCR_RAW_INDEX8: case OCR_RAW_GREY8: return width;
    case OCR_RAW_BGR555: case OCR_RAW_BGR565: case OCR_RAW_GREY16BE: return width * 2;
    case OCR_RAW_BGR24: case OCR_RAW_RGB24: return width * 3;
    case OCR_RAW_BGRX32: return width * 4;
    case OCR_RAW_RGB48BE: return width * 6;
    default: return 0;
  }
}
// the bytes of a (sound) frame that the kernel may read
size_t raw_need(const ocr_raw_frame& f) { return (size_t)(f.height - 1) * f.row_stride + raw_row_bytes(f.kind, (size_t)f.width); }

}  // namespace

const char* raw_frame_fault(const ocr_raw_frame& f) {
  if (f.kind < 0 || f.kind >= kRawKinds) return "raw frame: kind is not an ocr_raw_kind";
  if (f.width <= 0 || f.height <= 0 || (long)f.width * (long)f.height > (64L << 20)) return "raw frame: width and height must be positive and at most 64 Mpixel together";
  if (f.bottom_up != 0 && f.bottom_up != 1) return "raw frame: bottom_up must be 0 or 1";
  const size_t rb = raw_row_bytes(f.kind, (size_t)f.width);
  if (f.row_stride < rb) return "raw frame: row_stride is smaller than a row of this kind and width";
  if (f.row_stride > ((size_t)1 << 31)) return "raw frame: row_stride above 2 GiB";  // (times height < 2^26: raw_need cannot overflow)
  if (!f.data || f.data_len < raw_need(f)) return "raw frame: data_len is less than (height - 1) * row_stride + the last row";
  return nullptr;
}

void raw_relaunch(const RawScratch& sc, const RawLaunch& L, hipStream_t s) {
  for (int k = 0; k < kRawKinds; ++k)
    if (L.count[k] > 0) launch_raw(k, sc.id.p + L.first[k], L.count[k], L.units[k], s);
}

int raw_decode_async(const ocr_raw_frame* const* imgs, int count, uint8_t* const* dst, RawScratch& sc, hipStream_t s, std::string& err,
                     RawLaunch* launched) {
  std::vector<size_t> off((size_t)count);
  size_t bytes = 0;
  RawLaunch L;
  for (int i = 0; i < count; ++i) {
    if (!imgs[i]) { err = "null raw frame"; return OCR_ERR_ARG; }
    if (const char* fault = raw_frame_fault(*imgs[i])) { err = fault; return OCR_ERR_ARG; }
    off[i] = bytes;
    bytes += (raw_need(*imgs[i]) + 255) & ~(size_t)255;
    L.count[imgs[i]->kind]++;
  }
  L.bytes = bytes;
  if (!sc.data.ensure(bytes + 256, err) || !sc.id.ensure((size_t)count, err)) return OCR_ERR_DEVICE;
  if (!sc.stage.reserve(bytes, err)) return OCR_ERR_DEVICE;
  parallel_copy((size_t)count, bytes, [&](size_t i) { memcpy(sc.stage.p + off[i], imgs[i]->data, raw_need(*imgs[i])); });  // stored rows -> pinned memory
  // the descriptors ordered by the kernel that takes them, the units of a kind numbered through its frames
  for (int k = 1; k < kRawKinds; ++k) L.first[k] = L.first[k - 1] + L.count[k - 1];
  int next[kRawKinds];
  std::copy(L.first, L.first + kRawKinds, next);
  std::vector<RawImageDesc> id((size_t)count);
  for (int i = 0; i < count; ++i) {
    const ocr_raw_frame& f = *imgs[i];
    RawImageDesc& d = id[next[f.kind]++];
    memset(&d, 0, sizeof d);
    d.data = sc.data.p + off[i];
    d.bgr = dst[i];
    d.first_unit = L.units[f.kind];
    d.row_stride = f.row_stride;
    d.width = f.width; d.height = f.height; d.bottom_up = f.bottom_up;
    d.spans = raw_spans(f.width);
    L.units[f.kind] += (unsigned long long)f.height * d.spans;  // per frame < 2^32: height * ceil(width / 1024) <= 64M + height
    for (int k = 0; k < 256; ++k) d.palette[k] = (uint32_t)f.palette[4 * k] | ((uint32_t)f.palette[4 * k + 1] << 8) | ((uint32_t)f.palette[4 * k + 2] << 16);
  }
  if (!sc.stage.upload(sc.data.p, bytes, s, err) ||
      hipMemcpyAsync(sc.id.p, id.data(), id.size() * sizeof(RawImageDesc), hipMemcpyHostToDevice, s) != hipSuccess) {
    err = "raw rows upload failed";
    return OCR_ERR_DEVICE;
  }
  raw_relaunch(sc, L, s);
  if (launched) *launched = L;
  if (hipGetLastError() != hipSuccess) { err = "raw pixel kernels failed to launch"; return OCR_ERR_DEVICE; }
  return OCR_OK;
}

}  // namespace ocr

using namespace ocr;

namespace {
struct RawRoute : PlainRoute<ocr_raw_frame, RawScratch, RawLaunch, raw_frame_fault, raw_decode_async, raw_relaunch> {};
}  // namespace

extern "C" int ocr_raw_decode(const ocr_raw_frame* frame, int device_id, uint8_t* bgr, size_t cap) { return decode_frame<RawRoute>(frame, device_id, bgr, cap); }

extern "C" int ocr_raw_time(const ocr_raw_frame* frame, int device_id, int iters, double ms[2]) {
  if (!frame || !ms || iters <= 0) return fail(OCR_ERR_ARG, "null argument");
  return time_frames<RawRoute>(&frame, 1, device_id, iters, ms);
}

extern "C" int ocr_raw_time_batch(const ocr_raw_frame* const* frames, int count, int device_id, int iters, double ms[2]) {
  if (!frames || count < 1 || !ms || iters <= 0) return fail(OCR_ERR_ARG, "null argument");
  return time_frames<RawRoute>(frames, count, device_id, iters, ms);
}
