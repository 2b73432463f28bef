// Host side of the device TIFF back-end + its C-ABI entry points.  What is arithmetic about a batch - the rules of a frame, the
// image descriptors, the plan of a coded batch - is tiff_plan.h; here are the device calls around it.
#include <cstring>
#include <type_traits>

#include "capi_common.h"
#include "tiff_stage.h"

namespace ocr {

namespace tiff = PaddleOCR::tiff;
using tiff_plan::kCoded;
using tiff_plan::kDeflate;
using tiff_plan::kFax;

const char* tiff_frame_fault(const ocr_tiff_frame& f) {
  tiff::Geometry g;
  return tiff_plan::tiff_fault(f, g);
}

void tiff_relaunch(const TiffScratch& sc, const TiffLaunch& L, hipStream_t s) {
  for (int k = 0; k < kTiffKinds; ++k)
    if (L.count[k] > 0) launch_tiff(k, sc.id.p + L.first[k], L.count[k], L.units[k], s);
}

int tiff_decode_async(const ocr_tiff_frame* const* imgs, int count, uint8_t* const* dst, TiffScratch& sc, hipStream_t s, std::string& err,
                      TiffLaunch* launched) {
  std::vector<size_t> off((size_t)count);
  std::vector<tiff::Geometry> geo((size_t)count);
  size_t bytes = 0;
  TiffLaunch L;
  for (int i = 0; i < count; ++i) {
    if (!imgs[i]) { err = "null tiff frame"; return OCR_ERR_ARG; }
    if (const char* fault = tiff_plan::tiff_fault(*imgs[i], geo[i])) { err = fault; return OCR_ERR_ARG; }
    off[i] = bytes;
    bytes += tiff_plan::pad256(geo[i].total);
  }
  L.bytes = bytes;
  if (!sc.data.ensure(bytes + 256, err) || !sc.id.ensure((size_t)count, err)) return OCR_ERR_DEVICE;
  if (!sc.stage.reserve(bytes, err)) return OCR_ERR_DEVICE;
  parallel_copy((size_t)count, bytes, [&](size_t i) { memcpy(sc.stage.p + off[i], imgs[i]->data, geo[i].total); });  // chunks -> pinned memory
  const std::vector<TiffImageDesc> id = tiff_plan::describe(imgs, count, geo, off, dst, sc.data.p, L);
  if (!sc.stage.upload(sc.data.p, bytes, s, err) ||
      hipMemcpyAsync(sc.id.p, id.data(), id.size() * sizeof(TiffImageDesc), hipMemcpyHostToDevice, s) != hipSuccess) {
    err = "tiff chunks upload failed";
    return OCR_ERR_DEVICE;
  }
  tiff_relaunch(sc, L, s);
  if (launched) *launched = L;
  if (hipGetLastError() != hipSuccess) { err = "tiff pixel kernels failed to launch"; return OCR_ERR_DEVICE; }
  return OCR_OK;
}

const char* tiff_coded_fault(TiffRouteKind route, const ocr_tiff_coded& c) {
  tiff::Geometry g;
  return tiff_plan::coded_fault(route, c, g);
}

hipError_t tiff_middle_relaunch(TiffScratch& sc, const TiffLaunch& L, hipStream_t s) {
  if (L.route == kCoded) launch_tiff_expand((const TiffChunkDesc*)L.records, L.lzw, L.nrecords - L.lzw, L.pool, sc.data.p, s);
  else if (L.route == kFax) launch_tiff_fax((const TiffFaxDesc*)L.records, L.nrecords, L.pool, sc.data.p, s);
  else launch_inflate((const InflateDesc*)L.records, L.nrecords, L.pool, sc.data.p, sc.produced.p, s);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess || L.route != kDeflate) return e;
  // the counts of a Deflate batch, and the one wait of the coded routes
  if (L.nrecords) e = hipMemcpyAsync(sc.counts.p, sc.produced.p, (size_t)L.nrecords * 4, hipMemcpyDeviceToHost, s);
  return e != hipSuccess ? e : hipStreamSynchronize(s);
}

int tiff_coded_decode_async(TiffRouteKind route, const ocr_tiff_coded* const* imgs, int count, uint8_t* const* dst, TiffScratch& sc, hipStream_t s,
                            std::string& err, TiffLaunch* launched, bool pixels, uint32_t* const* produced, const int* ids) {
  static const char* const upload_failed[] = {"tiff coded chunks upload failed", "tiff deflate chunks upload failed", "tiff fax chunks upload failed"};
  static const char* const middle_failed[] = {"tiff expansion kernels failed to launch", "tiff inflate kernel failed", "tiff fax expansion kernel failed to launch"};
  static_assert(kCoded == 0 && kDeflate == 1 && kFax == 2, "the texts above are in the order of the routes");
  tiff_plan::Plan P;
  P.route = route;
  P.geo.resize((size_t)count);
  for (int i = 0; i < count; ++i) {
    if (!imgs[i]) { err = "null tiff frame"; return OCR_ERR_ARG; }
    if (const char* fault = tiff_plan::coded_fault(route, *imgs[i], P.geo[i])) { err = fault; return OCR_ERR_ARG; }
  }
  if (!tiff_plan::build(P, imgs, count)) { err = "tiff batch: more chunks than a launch has workgroups"; return OCR_ERR_ARG; }
  const size_t n = P.whose.size();
  TiffLaunch L;
  L.bytes = P.coded_bytes;
  if (!sc.data.ensure(P.bytes + 256, err) || !sc.coded.ensure(P.coded_bytes + 256, err) || !sc.id.ensure((size_t)count, err)) return OCR_ERR_DEVICE;
  if (route == kDeflate && !sc.produced.ensure(n + 1, err)) return OCR_ERR_DEVICE;
  if (!sc.stage.reserve(P.coded_bytes, err) || (route == kDeflate && !sc.counts.reserve((n + 1) * 4, err))) return OCR_ERR_DEVICE;
  if (n) memcpy(sc.stage.p, P.records(), P.record_bytes);
  parallel_copy((size_t)count, P.pool, [&](size_t i) { if (imgs[i]->bytes_len) memcpy(sc.stage.p + P.at_pool + P.pool_at[i], imgs[i]->bytes, imgs[i]->bytes_len); });
  L.route = route;
  L.records = sc.coded.p;
  L.nrecords = (uint32_t)n;
  L.lzw = P.lzw;
  L.pool = sc.coded.p + P.at_pool;
  const std::vector<TiffImageDesc> id = tiff_plan::describe(imgs, count, P.geo, P.off, dst, sc.data.p, L);
  if (!sc.stage.upload(sc.coded.p, P.coded_bytes, s, err) ||
      hipMemcpyAsync(sc.id.p, id.data(), id.size() * sizeof(TiffImageDesc), hipMemcpyHostToDevice, s) != hipSuccess) {
    err = upload_failed[route];
    return OCR_ERR_DEVICE;
  }
  if (tiff_middle_relaunch(sc, L, s) != hipSuccess) { err = middle_failed[route]; return OCR_ERR_DEVICE; }
  if (route == kDeflate) {  // (the counts are here: tiff_middle_relaunch waited for them)
    for (size_t k = 0; k < n; ++k) {
      const tiff_plan::Whose w = P.whose[k];
      if (produced && produced[w.frame]) produced[w.frame][w.chunk] = sc.produced_host()[k];
    }
    const size_t bad = pixels ? tiff_plan::first_short(P, sc.produced_host()) : n;
    if (bad < n) { err = tiff_plan::short_text(P, bad, ids); return OCR_ERR_ARG; }
  }
  if (pixels) {
    tiff_relaunch(sc, L, s);
    if (hipGetLastError() != hipSuccess) { err = "tiff pixel kernels failed to launch"; return OCR_ERR_DEVICE; }
  }
  if (launched) *launched = L;
  return OCR_OK;
}

}  // namespace ocr

using namespace ocr;

namespace {

struct TiffRoute : PlainRoute<ocr_tiff_frame, TiffScratch, TiffLaunch, tiff_frame_fault, tiff_decode_async, tiff_relaunch> {};

// a coded route: upload, the expansion of R (kDeflate: with its read-back), pixel stage
template <TiffRouteKind R>
struct TiffCodedRoute {
  using Frame = std::conditional_t<R == kFax, ocr_tiff_fax, ocr_tiff_coded>;
  using Scratch = TiffScratch;
  using Launch = TiffLaunch;
  static const ocr_tiff_coded& coded(const Frame& f) { return *(const ocr_tiff_coded*)&f; }  // (a fax frame starts with it)
  static const char* fault(const Frame& f) { return tiff_coded_fault(R, coded(f)); }
  static int rows(const Frame& f) { return coded(f).frame.height; }
  static int cols(const Frame& f) { return coded(f).frame.width; }
  static int decode(const Frame* const* frames, int count, uint8_t* const* dst, Scratch& sc, std::string& err, Launch* L) {
    return tiff_coded_decode_async(R, (const ocr_tiff_coded* const*)frames, count, dst, sc, nullptr, err, L);
  }
  static uint8_t* uploaded(Scratch& sc, const Launch&) { return sc.coded.p; }
  static hipError_t middle(Scratch& sc, const Launch& L) { return tiff_middle_relaunch(sc, L, nullptr); }
  static void pixels(Scratch& sc, const Launch& L) { tiff_relaunch(sc, L, nullptr); }
};

// ocr_tiff_expand, ocr_tiff_inflate, ocr_tiff_unfax: the expansion of one frame alone, its chunks to the caller's buffer
int expand_alone(TiffRouteKind route, const ocr_tiff_coded* coded, int device_id, uint8_t* out, size_t cap, uint32_t* produced) {
  if (!coded || !out) return fail(OCR_ERR_ARG, "null argument");
  tiff::Geometry g;
  if (const char* fault = tiff_plan::coded_fault(route, *coded, g)) return fail(OCR_ERR_ARG, fault);
  if (g.total > cap) return fail(OCR_ERR_CAPACITY, "output buffer too small");
  int rc = ocr_rt_init(device_id);
  if (rc) return rc;
  TiffScratch sc;
  std::string err;
  rc = tiff_coded_decode_async(route, &coded, 1, nullptr, sc, nullptr, err, nullptr, false, produced ? &produced : nullptr);
  if (rc) return fail(rc, err);
  CAPI_HIP(hipStreamSynchronize(nullptr));  // (a Deflate batch has waited for its counts already)
  CAPI_HIP(g_memcpy(out, sc.data.p, g.total, hipMemcpyDeviceToHost));
  return OCR_OK;
}

template <TiffRouteKind R>
int time_coded(const typename TiffCodedRoute<R>::Frame* const* frames, int count, int device_id, int iters, double ms[3]) {
  if (!frames || count < 1 || !frames[0] || !ms || iters <= 0) return fail(OCR_ERR_ARG, "null argument");
  return time_frames3<TiffCodedRoute<R>>(frames, count, device_id, iters, ms);
}

}  // namespace

extern "C" int ocr_tiff_expand(const ocr_tiff_coded* coded, int device_id, uint8_t* out, size_t cap) { return expand_alone(kCoded, coded, device_id, out, cap, nullptr); }
extern "C" int ocr_tiff_inflate(const ocr_tiff_coded* coded, int device_id, uint8_t* out, size_t cap, uint32_t* produced) {
  return expand_alone(kDeflate, coded, device_id, out, cap, produced);
}
extern "C" int ocr_tiff_unfax(const ocr_tiff_fax* fax, int device_id, uint8_t* out, size_t cap) {
  return expand_alone(kFax, (const ocr_tiff_coded*)fax, device_id, out, cap, nullptr);
}

extern "C" int ocr_tiff_decode_coded(const ocr_tiff_coded* coded, int device_id, uint8_t* bgr, size_t cap) {
  return decode_frame<TiffCodedRoute<kCoded>>(coded, device_id, bgr, cap);
}
extern "C" int ocr_tiff_decode_deflate(const ocr_tiff_coded* coded, int device_id, uint8_t* bgr, size_t cap) {
  return decode_frame<TiffCodedRoute<kDeflate>>(coded, device_id, bgr, cap);
}
extern "C" int ocr_tiff_decode_fax(const ocr_tiff_fax* fax, int device_id, uint8_t* bgr, size_t cap) {
  return decode_frame<TiffCodedRoute<kFax>>(fax, device_id, bgr, cap);
}

extern "C" int ocr_tiff_time_coded(const ocr_tiff_coded* coded, int device_id, int iters, double ms[3]) { return time_coded<kCoded>(&coded, 1, device_id, iters, ms); }
extern "C" int ocr_tiff_time_coded_batch(const ocr_tiff_coded* const* coded, int count, int device_id, int iters, double ms[3]) {
  return time_coded<kCoded>(coded, count, device_id, iters, ms);
}
extern "C" int ocr_tiff_time_deflate(const ocr_tiff_coded* coded, int device_id, int iters, double ms[3]) { return time_coded<kDeflate>(&coded, 1, device_id, iters, ms); }
extern "C" int ocr_tiff_time_deflate_batch(const ocr_tiff_coded* const* coded, int count, int device_id, int iters, double ms[3]) {
  return time_coded<kDeflate>(coded, count, device_id, iters, ms);
}
extern "C" int ocr_tiff_time_fax(const ocr_tiff_fax* fax, int device_id, int iters, double ms[3]) { return time_coded<kFax>(&fax, 1, device_id, iters, ms); }
extern "C" int ocr_tiff_time_fax_batch(const ocr_tiff_fax* const* fax, int count, int device_id, int iters, double ms[3]) {
  return time_coded<kFax>(fax, count, device_id, iters, ms);
}

extern "C" int ocr_tiff_decode(const ocr_tiff_frame* frame, int device_id, uint8_t* bgr, size_t cap) { return decode_frame<TiffRoute>(frame, device_id, bgr, cap); }

extern "C" int ocr_tiff_time(const ocr_tiff_frame* frame, int device_id, int iters, double ms[2]) {
  if (!frame || !ms || iters <= 0) return fail(OCR_ERR_ARG, "null argument");
  return time_frames<TiffRoute>(&frame, 1, device_id, iters, ms);
}

extern "C" int ocr_tiff_time_batch(const ocr_tiff_frame* const* frames, int count, int device_id, int iters, double ms[2]) {
  if (!frames || count < 1 || !ms || iters <= 0) return fail(OCR_ERR_ARG, "null argument");
  return time_frames<TiffRoute>(frames, count, device_id, iters, ms);
}

// measurement aid (decode_tool --time): the device time of one plain copy KERNEL over `bytes` (16 bytes a lane, grid stride:
// launch_plain_copy), the yardstick the pixel stage's time is set against in the same run
extern "C" int ocr_dev_copy_time(void* dst, const void* src, size_t bytes, int iters, double* ms) {
  if (!dst || !src || !ms || iters <= 0 || bytes < 16 || (((uintptr_t)dst | (uintptr_t)src) & 15)) return fail(OCR_ERR_ARG, "null, unaligned or empty argument");
  launch_plain_copy(dst, src, bytes, nullptr);  // (the first launch is not timed)
  double t[2];
  const int rc = time_phases(iters, t, [&] { launch_plain_copy(dst, src, bytes, nullptr); return hipGetLastError(); }, [] { return hipSuccess; });
  if (rc == OCR_OK) *ms = t[0];
  return rc;
}
