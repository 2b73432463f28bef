// Host side of the device VP8 (lossy WebP) back-end + its C-ABI entry points.
#include <algorithm>
#include <cstring>

#include "capi_common.h"
#include "vp8_stage.h"

namespace ocr {

namespace {

using PaddleOCR::vp8::Mb;
static_assert(sizeof(ocr_vp8_mb) == sizeof(Mb) && offsetof(ocr_vp8_mb, nz_y) == offsetof(Mb, nz_y) && offsetof(ocr_vp8_mb, level) == offsetof(Mb, level) &&
                  offsetof(ocr_vp8_mb, coeff_off) == offsetof(Mb, coeff_off),
              "ocr_vp8_mb is vp8::Mb");

size_t pad256(size_t bytes) { return (bytes + 255) & ~(size_t)255; }
size_t mb_count(const ocr_vp8_frame& f) { return (size_t)((f.width + 15) >> 4) * ((f.height + 15) >> 4); }

}  // namespace

// host/vp8_decode.h fault_of(): the one statement of the rules
const char* vp8_frame_fault(const ocr_vp8_frame& f) {
  if (f.mbs && !f.coeffs && f.coeffs_len) return "vp8 frame: coefficients are missing";
  return PaddleOCR::vp8::fault_of(f.width, f.height, f.filter_type, (const Mb*)f.mbs, f.mbs_len, f.coeffs ? f.coeffs_len : 0);
}

void vp8_relaunch(const Vp8Scratch& sc, const Vp8Launch& L, hipStream_t s) { launch_vp8(sc.id.p, L.count, L.any_filter, L.max_units, s); }

int vp8_decode_async(const ocr_vp8_frame* const* imgs, int count, uint8_t* const* dst, Vp8Scratch& sc, hipStream_t s, std::string& err,
                     Vp8Launch* launched) {
  struct Place { size_t mbs = 0, coeffs = 0, planes = 0; };
  std::vector<Place> at((size_t)count);
  size_t bytes = 0, planes = 0;
  Vp8Launch L;
  L.count = count;
  for (int i = 0; i < count; ++i) {
    if (!imgs[i]) { err = "null vp8 frame"; return OCR_ERR_ARG; }
    if (const char* fault = vp8_frame_fault(*imgs[i])) { err = fault; return OCR_ERR_ARG; }
    const size_t n = mb_count(*imgs[i]);
    at[i].mbs = bytes;
    bytes += pad256(n * sizeof(Mb));
    at[i].coeffs = bytes;
    bytes += pad256(imgs[i]->coeffs_len * 2);
    at[i].planes = planes;
    planes += n * 384;  // 256 luma + 2 x 64 chroma bytes a macroblock: every plane starts on a multiple of 64
    L.any_filter |= imgs[i]->filter_type != 0;
  }
  L.bytes = bytes;
  if (!sc.data.ensure(bytes + 256, err) || !sc.planes.ensure(planes + 256, err) || !sc.id.ensure((size_t)count, err)) return OCR_ERR_DEVICE;
  if (!sc.stage.reserve(bytes + 256, err)) return OCR_ERR_DEVICE;
  parallel_copy((size_t)count, bytes, [&](size_t i) {  // descriptors -> pinned memory
    const ocr_vp8_frame& f = *imgs[i];
    memcpy(sc.stage.p + at[i].mbs, f.mbs, mb_count(f) * sizeof(Mb));
    if (f.coeffs_len) memcpy(sc.stage.p + at[i].coeffs, f.coeffs, f.coeffs_len * 2);
  });
  std::vector<Vp8ImageDesc> id((size_t)count);
  for (int i = 0; i < count; ++i) {
    const ocr_vp8_frame& f = *imgs[i];
    const size_t n = mb_count(f);
    Vp8ImageDesc& d = id[(size_t)i];
    memset(&d, 0, sizeof d);
    d.mbs = (const Mb*)(sc.data.p + at[i].mbs);
    d.coeffs = (const int16_t*)(sc.data.p + at[i].coeffs);
    d.y = sc.planes.p + at[i].planes;
    d.u = d.y + n * 256;
    d.v = d.u + n * 64;
    d.bgr = dst[i];
    d.width = f.width; d.height = f.height;
    d.mb_w = (f.width + 15) >> 4; d.mb_h = (f.height + 15) >> 4;
    d.filter_type = f.filter_type;
    const size_t npx = (size_t)f.width * f.height, head = std::min<size_t>(npx, (size_t)((uintptr_t)dst[i] & 3));
    d.units = (unsigned)(1 + (npx - head + kVp8Group - 1) / kVp8Group);
    L.max_units = std::max(L.max_units, d.units);
  }
  if (!sc.stage.upload(sc.data.p, bytes, s, err) ||
      hipMemcpyAsync(sc.id.p, id.data(), id.size() * sizeof(Vp8ImageDesc), hipMemcpyHostToDevice, s) != hipSuccess) {
    err = "vp8 descriptor upload failed";
    return OCR_ERR_DEVICE;
  }
  vp8_relaunch(sc, L, s);
  if (launched) *launched = L;
  if (hipGetLastError() != hipSuccess) { err = "vp8 pixel kernels failed to launch"; return OCR_ERR_DEVICE; }
  return OCR_OK;
}

}  // namespace ocr

using namespace ocr;

namespace {
struct Vp8Route : PlainRoute<ocr_vp8_frame, Vp8Scratch, Vp8Launch, vp8_frame_fault, vp8_decode_async, vp8_relaunch> {};
}  // namespace

extern "C" int ocr_vp8_decode(const ocr_vp8_frame* frame, int device_id, uint8_t* bgr, size_t cap) { return decode_frame<Vp8Route>(frame, device_id, bgr, cap); }

extern "C" int ocr_vp8_time(const ocr_vp8_frame* frame, int device_id, int iters, double ms[2]) {
  if (!frame || !ms || iters <= 0) return fail(OCR_ERR_ARG, "null argument");
  return time_frames<Vp8Route>(&frame, 1, device_id, iters, ms);
}

extern "C" int ocr_vp8_time_batch(const ocr_vp8_frame* const* frames, int count, int device_id, int iters, double ms[2]) {
  if (!frames || count < 1 || !ms || iters <= 0) return fail(OCR_ERR_ARG, "null argument");
  return time_frames<Vp8Route>(frames, count, device_id, iters, ms);
}
