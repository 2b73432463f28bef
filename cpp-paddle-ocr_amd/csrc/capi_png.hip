// Host side of the device PNG back-end + its C-ABI entry points.
#include <algorithm>
#include <cstring>

#include "capi_common.h"
#include "png_stage.h"

namespace ocr {

namespace {

// host/png_decode.h geometry(): the passes of an image and the size of its inflated stream; false = not a legal header
bool png_geometry(const ocr_png_frame& f, PngPassDesc pass[7], int& npass, size_t& total) {
  const long w = f.width, h = f.height;
  if (w <= 0 || h <= 0 || w * h > (64L << 20)) return false;
  const int d = f.bit_depth;
  int channels;
  switch (f.color_type) {
    case 0: channels = 1; if (d != 1 && d != 2 && d != 4 && d != 8 && d != 16) return false; break;
    case 3: channels = 1; if (d != 1 && d != 2 && d != 4 && d != 8) return false; break;
    case 2: channels = 3; if (d != 8 && d != 16) return false; break;
    case 4: channels = 2; if (d != 8 && d != 16) return false; break;
    case 6: channels = 4; if (d != 8 && d != 16) return false; break;
    default: return false;
  }
  if (f.interlace != 0 && f.interlace != 1) return false;
  static const int X0[7] = {0, 4, 0, 2, 0, 1, 0}, Y0[7] = {0, 0, 4, 0, 2, 0, 1}, DX[7] = {8, 8, 4, 4, 2, 2, 1}, DY[7] = {8, 8, 8, 4, 4, 2, 2};
  npass = f.interlace ? 7 : 1;
  total = 0;
  for (int p = 0; p < npass; ++p) {
    PngPassDesc& q = pass[p];
    q = PngPassDesc{};
    q.dx = q.dy = 1;
    if (f.interlace) { q.x0 = X0[p]; q.y0 = Y0[p]; q.dx = DX[p]; q.dy = DY[p]; }
    q.cols = w > q.x0 ? (int)((w - q.x0 + q.dx - 1) / q.dx) : 0;
    q.rows = h > q.y0 ? (int)((h - q.y0 + q.dy - 1) / q.dy) : 0;
    if (q.cols == 0 || q.rows == 0) q.cols = q.rows = 0;
    q.rowbytes = (int)(((size_t)q.cols * channels * d + 7) / 8);  // <= 64M pixels * 8 bytes
    q.offset = total;
    if (q.rows) total += (size_t)q.rows * (1 + (size_t)q.rowbytes);
  }
  return true;
}

int png_bpp(const ocr_png_frame& f) {
  const int channels = f.color_type == 2 ? 3 : f.color_type == 4 ? 2 : f.color_type == 6 ? 4 : 1, bits = channels * f.bit_depth;
  return bits < 8 ? 1 : bits / 8;
}

}  // namespace

const char* png_frame_fault(const ocr_png_frame& f) {
  if (f.reserved != 0) return "PNG frame: reserved must be 0";
  PngPassDesc pass[7];
  int npass;
  size_t total;
  if (!png_geometry(f, pass, npass, total)) return "PNG frame: size, colour type, bit depth or interlace outside what PNG allows (at most 64 Mpixel)";
  if (!f.data || f.data_len != total) return "PNG frame: data_len is not what the header implies";
  if (!f.segments || f.nsegments < 1) return "PNG frame: no segment table";
  // a segment is serial work for one wave, a table entry a workgroup: bounds on both (host/png_decode.h finishes such files on the host)
  if (f.nsegments > kPngMaxSegments) return "PNG frame: more segments than the device stage takes (65536)";
  for (int p = 0; p < npass; ++p)
    if (pass[p].rows > kPngMaxRows) return "PNG frame: more rows in a pass than the device stage takes (16384)";
  int k = 0;
  for (int p = 0; p < npass; ++p) {
    const PngPassDesc& q = pass[p];
    const size_t stride = 1 + (size_t)q.rowbytes;
    for (int r = 0; r < q.rows;) {
      if (k >= f.nsegments) return "PNG frame: the segments do not cover every row";
      const ocr_png_segment& s = f.segments[k++];
      if (s.pass != p || s.first_row != r || s.rows < 1 || s.rows > q.rows - r) return "PNG frame: the segments do not tile the rows in order";
      for (int i = 0; i < s.rows; ++i) {
        const uint8_t ft = f.data[q.offset + (size_t)(r + i) * stride];
        if (ft > 4) return "PNG frame: filter byte above 4";
        if (i == 0 && r != 0 && ft > 1) return "PNG frame: a segment starts at a row that needs the row above";
      }
      r += s.rows;
    }
  }
  if (k != f.nsegments) return "PNG frame: segments beyond the last row";
  return nullptr;
}

void png_relaunch(const PngScratch& sc, const PngLaunch& L, hipStream_t s) {
  for (int k = 0; k < kPngKinds; ++k)
    if (L.count[k] > 0) launch_png(k, sc.id.p, sc.work.p + L.first[k], L.count[k], s);
}

int png_decode_async(const ocr_png_frame* const* imgs, int count, uint8_t* const* dst, PngScratch& sc, hipStream_t s, std::string& err,
                     PngLaunch* launched) {
  std::vector<size_t> off((size_t)count);
  size_t bytes = 0;
  for (int i = 0; i < count; ++i) {
    if (!imgs[i]) { err = "null PNG frame"; return OCR_ERR_ARG; }
    if (const char* fault = png_frame_fault(*imgs[i])) { err = fault; return OCR_ERR_ARG; }
    off[i] = bytes;
    bytes += (imgs[i]->data_len + 255) & ~(size_t)255;
  }
  PngLaunch L;
  L.bytes = bytes;
  std::vector<PngImageDesc> id((size_t)count);
  std::vector<int> kinds((size_t)count);
  size_t nwork = 0;
  for (int i = 0; i < count; ++i) {
    kinds[i] = png_kind(png_bpp(*imgs[i]));
    L.count[kinds[i]] += imgs[i]->nsegments;
    nwork += (size_t)imgs[i]->nsegments;
  }
  if (!sc.data.ensure(bytes + 256, err) || !sc.recon.ensure(bytes + 256, err) || !sc.id.ensure((size_t)count, err) || !sc.work.ensure(nwork, err))
    return OCR_ERR_DEVICE;
  if (!sc.stage.reserve(bytes, err)) return OCR_ERR_DEVICE;
  parallel_copy((size_t)count, bytes, [&](size_t i) { memcpy(sc.stage.p + off[i], imgs[i]->data, imgs[i]->data_len); });  // inflated streams -> pinned memory
  // the segments ordered by the kernel that takes them
  for (int k = 1; k < kPngKinds; ++k) L.first[k] = L.first[k - 1] + L.count[k - 1];
  int next[kPngKinds];
  std::copy(L.first, L.first + kPngKinds, next);
  std::vector<PngWork> work(nwork);
  for (int i = 0; i < count; ++i) {
    const ocr_png_frame& f = *imgs[i];
    PngImageDesc& d = id[i];
    memset(&d, 0, sizeof d);
    int npass;
    size_t total;
    png_geometry(f, d.pass, npass, total);
    d.data = sc.data.p + off[i];
    d.recon = sc.recon.p + off[i];
    d.bgr = dst[i];
    d.width = f.width; d.height = f.height; d.depth = f.bit_depth; d.ctype = f.color_type;
    memcpy(d.palette, f.palette, sizeof d.palette);
    for (int j = 0; j < f.nsegments; ++j) work[next[kinds[i]]++] = PngWork{i, f.segments[j].pass, f.segments[j].first_row, f.segments[j].rows};
  }
  if (!sc.stage.upload(sc.data.p, bytes, s, err) ||
      hipMemcpyAsync(sc.id.p, id.data(), id.size() * sizeof(PngImageDesc), hipMemcpyHostToDevice, s) != hipSuccess ||
      hipMemcpyAsync(sc.work.p, work.data(), work.size() * sizeof(PngWork), hipMemcpyHostToDevice, s) != hipSuccess) {
    err = "PNG stream upload failed";
    return OCR_ERR_DEVICE;
  }
  png_relaunch(sc, L, s);
  if (launched) *launched = L;
  if (hipGetLastError() != hipSuccess) { err = "PNG kernels failed to launch"; return OCR_ERR_DEVICE; }
  return OCR_OK;
}

}  // namespace ocr

using namespace ocr;

namespace {
struct PngRoute : PlainRoute<ocr_png_frame, PngScratch, PngLaunch, png_frame_fault, png_decode_async, png_relaunch> {};
}  // namespace

extern "C" int ocr_png_decode(const ocr_png_frame* frame, int device_id, uint8_t* bgr, size_t cap) { return decode_frame<PngRoute>(frame, device_id, bgr, cap); }

extern "C" int ocr_png_time(const ocr_png_frame* frame, int device_id, int iters, double ms[2]) {
  if (!frame || !ms || iters <= 0) return fail(OCR_ERR_ARG, "null argument");
  return time_frames<PngRoute>(&frame, 1, device_id, iters, ms);
}

extern "C" int ocr_png_time_batch(const ocr_png_frame* const* frames, int count, int device_id, int iters, double ms[2]) {
  if (!frames || count < 1 || !ms || iters <= 0) return fail(OCR_ERR_ARG, "null argument");
  return time_frames<PngRoute>(frames, count, device_id, iters, ms);
}
