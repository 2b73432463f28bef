// Host side of the device WebP back-end + its C-ABI entry points.
#include <algorithm>
#include <cstring>

#include "capi_common.h"
#include "webp_stage.h"

namespace ocr {

namespace {

// host/webp_decode.h: what follows from a (sound) descriptor
struct WebpGeometry {
  int coded_width = 0, pred = -1, cross = -1, index = -1;  // positions of the transforms in the file, -1: absent
  size_t sub[4] = {};                                       // dwords of each transform's data the kernels read
};

// host/webp_decode.h fault(), rule for rule, and the device scope behind it
const char* webp_fault(const ocr_webp_frame& f, WebpGeometry& g) {
  if (f.width <= 0 || f.height <= 0 || f.width > 16384 || f.height > 16384 || (long)f.width * f.height > (64L << 20))
    return "webp frame: width and height must be 1 .. 16384 and at most 64 Mpixel together";
  if (f.ntransforms < 0 || f.ntransforms > 4) return "webp frame: at most four transforms";
  unsigned seen = 0;
  int w = f.width;
  for (int t = 0; t < f.ntransforms; ++t) {
    const auto& tr = f.transforms[t];
    if (tr.kind < 0 || tr.kind > 3) return "webp frame: transform kind must be 0 .. 3";
    if (seen & (1u << tr.kind)) return "webp frame: a transform kind occurs twice";
    seen |= 1u << tr.kind;
    if (tr.kind == 0 || tr.kind == 1) {
      if (tr.bits < 2 || tr.bits > 9) return "webp frame: block bits must be 2 .. 9";
      const int m = (1 << tr.bits) - 1;
      g.sub[t] = (size_t)((w + m) >> tr.bits) * ((f.height + m) >> tr.bits);
      if (!tr.data || tr.data_len < g.sub[t]) return "webp frame: a transform's sub-image is smaller than its blocks";
      (tr.kind == 0 ? g.pred : g.cross) = t;
    } else if (tr.kind == 2) {
      if (tr.bits != 0) return "webp frame: add-green has no bits";
    } else {
      if (!tr.data || tr.data_len < 1 || tr.data_len > 256) return "webp frame: the palette has 1 .. 256 entries";
      const int bits = tr.data_len > 16 ? 0 : tr.data_len > 4 ? 1 : tr.data_len > 2 ? 2 : 3;
      if (tr.bits != bits) return "webp frame: the bundling bits do not follow from the palette size";
      if (t != 0) return "webp frame: colour indexing must be the first transform of the file for the device stage";
      g.index = t;
      g.sub[t] = tr.data_len;
      w = (w + (1 << bits) - 1) >> bits;
    }
  }
  g.coded_width = w;
  if (!f.argb || f.argb_len < (size_t)w * f.height) return "webp frame: fewer coded pixels than coded width x height";
  return nullptr;
}

size_t pad256(size_t bytes) { return (bytes + 255) & ~(size_t)255; }

}  // namespace

const char* webp_frame_fault(const ocr_webp_frame& f) {
  WebpGeometry g;
  return webp_fault(f, g);
}

void webp_relaunch(const WebpScratch& sc, const WebpLaunch& L, hipStream_t s) {
  for (int k = 0; k < kWebpKinds; ++k)
    if (L.count[k] > 0) launch_webp(k, sc.id.p + L.first[k], L.count[k], L.units, s);
}

int webp_decode_async(const ocr_webp_frame* const* imgs, int count, uint8_t* const* dst, WebpScratch& sc, hipStream_t s, std::string& err,
                      WebpLaunch* launched) {
  std::vector<WebpGeometry> geo((size_t)count);
  // per image: where the coded image and the two sub-images lie in the upload, and its replayed rows
  struct Place { size_t argb = 0, pred = 0, cross = 0, recon = 0; };
  std::vector<Place> at((size_t)count);
  size_t bytes = 0, recon = 0;
  WebpLaunch L;
  for (int i = 0; i < count; ++i) {
    if (!imgs[i]) { err = "null webp frame"; return OCR_ERR_ARG; }
    if (const char* fault = webp_fault(*imgs[i], geo[i])) { err = fault; return OCR_ERR_ARG; }
    const WebpGeometry& g = geo[i];
    at[i].argb = bytes;
    bytes += pad256((size_t)g.coded_width * imgs[i]->height * 4);
    if (g.pred >= 0) { at[i].pred = bytes; bytes += pad256(g.sub[g.pred] * 4); }
    if (g.cross >= 0) { at[i].cross = bytes; bytes += pad256(g.sub[g.cross] * 4); }
    at[i].recon = recon;
    if (g.pred >= 0) recon += (size_t)webp_recon_rows(imgs[i]->height) * g.coded_width;
    L.count[g.pred >= 0 ? 0 : 1]++;
  }
  L.bytes = bytes;
  if (!sc.data.ensure(bytes + 256, err) || !sc.recon.ensure(recon + 64, err) || !sc.id.ensure((size_t)count, err)) return OCR_ERR_DEVICE;
  if (!sc.stage.reserve(bytes, err)) return OCR_ERR_DEVICE;
  parallel_copy((size_t)count, bytes, [&](size_t i) {  // coded data -> pinned memory
    const ocr_webp_frame& f = *imgs[i];
    const WebpGeometry& g = geo[i];
    memcpy(sc.stage.p + at[i].argb, f.argb, (size_t)g.coded_width * f.height * 4);
    if (g.pred >= 0) memcpy(sc.stage.p + at[i].pred, f.transforms[g.pred].data, g.sub[g.pred] * 4);
    if (g.cross >= 0) memcpy(sc.stage.p + at[i].cross, f.transforms[g.cross].data, g.sub[g.cross] * 4);
  });
  L.first[1] = L.count[0];
  int next[kWebpKinds] = {L.first[0], L.first[1]};
  std::vector<WebpImageDesc> id((size_t)count);
  for (int i = 0; i < count; ++i) {
    const ocr_webp_frame& f = *imgs[i];
    const WebpGeometry& g = geo[i];
    const int kind = g.pred >= 0 ? 0 : 1;
    WebpImageDesc& d = id[next[kind]++];
    memset(&d, 0, sizeof d);
    d.argb = (const uint32_t*)(sc.data.p + at[i].argb);
    d.pred = g.pred >= 0 ? (const uint32_t*)(sc.data.p + at[i].pred) : nullptr;
    d.cross = g.cross >= 0 ? (const uint32_t*)(sc.data.p + at[i].cross) : nullptr;
    d.recon = sc.recon.p + at[i].recon;
    d.bgr = dst[i];
    d.width = f.width; d.height = f.height; d.coded_width = g.coded_width;
    d.pred_bits = g.pred >= 0 ? f.transforms[g.pred].bits : 0;
    d.cross_bits = g.cross >= 0 ? f.transforms[g.cross].bits : 0;
    d.index_bits = g.index >= 0 ? f.transforms[g.index].bits : -1;
    // the transforms are undone last to first: what stands behind the predictor in the file is undone in front of it
    for (int t = f.ntransforms - 1; t >= 0; --t) {
      const int k = f.transforms[t].kind;
      if (k != 1 && k != 2) continue;
      const int op = k == 1 ? WEBP_OP_CROSS : WEBP_OP_GREEN;
      if (g.pred < 0 || t > g.pred) d.pre[d.npre++] = op;
      else d.post[d.npost++] = op;
    }
    if (g.index >= 0)
      for (size_t k = 0; k < f.transforms[g.index].data_len; ++k) d.palette[k] = f.transforms[g.index].data[k] & 0xFFFFFFu;
    if (kind == 1) {
      d.spans = (unsigned)((f.width + 3 + kWebpBlock * kWebpGroup - 1) / (kWebpBlock * kWebpGroup));  // (+ 3: the head shifts the groups)
      d.first_unit = L.units;
      L.units += (unsigned long long)d.spans * f.height;
    }
  }
  if (!sc.stage.upload(sc.data.p, bytes, s, err) ||
      hipMemcpyAsync(sc.id.p, id.data(), id.size() * sizeof(WebpImageDesc), hipMemcpyHostToDevice, s) != hipSuccess) {
    err = "webp coded data upload failed";
    return OCR_ERR_DEVICE;
  }
  webp_relaunch(sc, L, s);
  if (launched) *launched = L;
  if (hipGetLastError() != hipSuccess) { err = "webp pixel kernels failed to launch"; return OCR_ERR_DEVICE; }
  return OCR_OK;
}

}  // namespace ocr

using namespace ocr;

namespace {
struct WebpRoute : PlainRoute<ocr_webp_frame, WebpScratch, WebpLaunch, webp_frame_fault, webp_decode_async, webp_relaunch> {};
}  // namespace

extern "C" int ocr_webp_decode(const ocr_webp_frame* frame, int device_id, uint8_t* bgr, size_t cap) { return decode_frame<WebpRoute>(frame, device_id, bgr, cap); }

extern "C" int ocr_webp_time(const ocr_webp_frame* frame, int device_id, int iters, double ms[2]) {
  if (!frame || !ms || iters <= 0) return fail(OCR_ERR_ARG, "null argument");
  return time_frames<WebpRoute>(&frame, 1, device_id, iters, ms);
}

extern "C" int ocr_webp_time_batch(const ocr_webp_frame* const* frames, int count, int device_id, int iters, double ms[2]) {
  if (!frames || count < 1 || !ms || iters <= 0) return fail(OCR_ERR_ARG, "null argument");
  return time_frames<WebpRoute>(frames, count, device_id, iters, ms);
}
