// Host side of the device JPEG back-end + its C-ABI test entry point.
#include <algorithm>
#include <cstddef>
#include <cstring>

#include "capi_common.h"
#include "jpeg_stage.h"

namespace ocr {

// orientation took the place of alignment padding: callers built against the header without it keep their layout
static_assert(sizeof(ocr_jpeg_img) == 24 + 3 * sizeof(ocr_jpeg_comp) && offsetof(ocr_jpeg_img, comp) == 24, "ocr_jpeg_img layout");

bool jpeg_img_valid(const ocr_jpeg_img& im) {
  if (im.orientation < 0 || im.orientation > 8) return false;
  if (im.rows <= 0 || im.cols <= 0 || (long)im.rows * im.cols > (64L << 20) || (im.ncomp != 1 && im.ncomp != 3)) return false;
  const bool s444 = im.hmax == 1 && im.vmax == 1, s422 = im.hmax == 2 && im.vmax == 1, s420 = im.hmax == 2 && im.vmax == 2;
  if (!(s444 || s422 || s420) || (im.ncomp == 1 && !s444)) return false;
  for (int c = 0; c < im.ncomp; ++c) {
    const ocr_jpeg_comp& k = im.comp[c];
    const int h = c == 0 ? im.hmax : 1, v = c == 0 ? im.vmax : 1;
    if (!k.coef || k.bw <= 0 || k.bh <= 0) return false;
    if (k.dw != (im.cols * h + im.hmax - 1) / im.hmax || k.dh != (im.rows * v + im.vmax - 1) / im.vmax) return false;
    if (k.bw * 8 < k.dw || k.bh * 8 < k.dh || k.bw > 16384 || k.bh > 16384) return false;  // the planes cover the component
  }
  return true;
}

namespace {
struct FrameMax { int hmax = 1, vmax = 1; };
FrameMax frame_max(const ocr_jpeg_frame& f) {
  FrameMax m;
  for (int c = 0; c < f.ncomp; ++c) { m.hmax = std::max(m.hmax, f.comp[c].h); m.vmax = std::max(m.vmax, f.comp[c].v); }
  return m;
}
}  // namespace

const char* jpeg_frame_fault(const ocr_jpeg_frame& f) {
  if (f.orientation < 0 || f.orientation > 8) return "JPEG frame: orientation outside 0..8";
  if (f.reserved != 0) return "JPEG frame: reserved must be 0";
  if (f.rows <= 0 || f.cols <= 0 || (long)f.rows * f.cols > (64L << 20)) return "JPEG frame: size outside 1 .. 64 Mpixel";
  if (f.ncomp != 1 && f.ncomp != 3 && f.ncomp != 4) return "JPEG frame: ncomp must be 1, 3 or 4";
  const bool color_ok = f.ncomp == 1 ? f.color == OCR_JPEG_GREY
                      : f.ncomp == 3 ? (f.color == OCR_JPEG_YCBCR || f.color == OCR_JPEG_RGB) : (f.color == OCR_JPEG_CMYK || f.color == OCR_JPEG_YCCK);
  if (!color_ok) return "JPEG frame: colour space does not fit the number of components";
  for (int c = 0; c < f.ncomp; ++c)
    if (f.comp[c].h < 1 || f.comp[c].h > 4 || f.comp[c].v < 1 || f.comp[c].v > 4) return "JPEG frame: sampling factor outside 1..4";
  if (f.ncomp == 1 && (f.comp[0].h != 1 || f.comp[0].v != 1)) return "JPEG frame: a single component has factors 1x1";
  const FrameMax m = frame_max(f);
  for (int c = 0; c < f.ncomp; ++c) {
    const ocr_jpeg_fcomp& k = f.comp[c];
    if (m.hmax % k.h != 0 || m.vmax % k.v != 0) return "JPEG frame: fractional upsampling (hmax / h or vmax / v not integral)";
    if (!k.coef || k.bw <= 0 || k.bh <= 0) return "JPEG frame: component without coefficients";
    if (k.dw != (int)(((long)f.cols * k.h + m.hmax - 1) / m.hmax) || k.dh != (int)(((long)f.rows * k.v + m.vmax - 1) / m.vmax))
      return "JPEG frame: dw / dh are not ceil(cols*h/hmax), ceil(rows*v/vmax)";
    if ((long)k.bw * 8 < k.dw || (long)k.bh * 8 < k.dh || k.bw > 16384 || k.bh > 16384) return "JPEG frame: the blocks do not cover the component";
  }
  return nullptr;
}

ocr_jpeg_frame jpeg_frame_of(const ocr_jpeg_img& im) {
  ocr_jpeg_frame f;
  memset(&f, 0, sizeof f);
  f.rows = im.rows; f.cols = im.cols; f.ncomp = im.ncomp; f.orientation = im.orientation;
  f.color = im.ncomp == 1 ? OCR_JPEG_GREY : OCR_JPEG_YCBCR;
  for (int c = 0; c < im.ncomp && c < 3; ++c) {
    const ocr_jpeg_comp& k = im.comp[c];
    ocr_jpeg_fcomp& o = f.comp[c];
    o.coef = k.coef;
    memcpy(o.quant, k.quant, sizeof o.quant);
    o.bw = k.bw; o.bh = k.bh; o.dw = k.dw; o.dh = k.dh;
    o.h = c == 0 ? im.hmax : 1; o.v = c == 0 ? im.vmax : 1;
  }
  return f;
}

// What the kernels of the first three kinds compute: grey, or YCbCr with luma at the maximum factors 1x1 / 2x1 / 2x2 and
// both chroma 1x1 - and more than 2 samples wide when they are subsampled: jdsample.c replicates a narrower component
// where those kernels interpolate, so such an image (at most 4 pixels wide) is one of the general kinds.
int jpeg_frame_kind(const ocr_jpeg_frame& f) {
  bool classic = f.ncomp == 1;
  if (f.ncomp == 3 && f.color == OCR_JPEG_YCBCR) {
    const FrameMax m = frame_max(f);
    const bool s444 = m.hmax == 1 && m.vmax == 1, s422 = m.hmax == 2 && m.vmax == 1, s420 = m.hmax == 2 && m.vmax == 2;
    classic = (s444 || s422 || s420) && f.comp[0].h == m.hmax && f.comp[0].v == m.vmax && f.comp[1].h == 1 && f.comp[1].v == 1 &&
              f.comp[2].h == 1 && f.comp[2].v == 1 && (s444 || f.comp[1].dw > 2);
  }
  return classic ? jpeg_output_kind(f.orientation) : jpeg_general_kind(f.orientation);
}

int jpeg_decode_async(const ocr_jpeg_frame* const* imgs, int count, uint8_t* const* dst, JpegScratch& sc, hipStream_t s, std::string& err,
                      JpegLaunch* launched) {
  std::vector<JpegPlaneDesc> pd;
  std::vector<size_t> coef_off, plane_off;
  size_t ncoef = 0, nplane = 0;
  long nblocks = 0;
  JpegLaunch L;
  std::vector<int> kinds((size_t)count);
  for (int i = 0; i < count; ++i) {
    const ocr_jpeg_frame& im = *imgs[i];
    if (const char* fault = jpeg_frame_fault(im)) { err = fault; return OCR_ERR_ARG; }
    kinds[i] = jpeg_frame_kind(im);
    L.count[kinds[i]]++;
    for (int c = 0; c < im.ncomp; ++c) {
      const ocr_jpeg_fcomp& k = im.comp[c];
      JpegPlaneDesc d{};
      memcpy(d.quant, k.quant, sizeof d.quant);
      d.bw = k.bw; d.bh = k.bh; d.first_block = nblocks;
      pd.push_back(d);
      coef_off.push_back(ncoef);
      plane_off.push_back(nplane);
      ncoef += (size_t)k.bw * k.bh * 64;
      nplane += ((size_t)k.bw * 8 * k.bh * 8 + 255) & ~(size_t)255;
      nblocks += (long)k.bw * k.bh;
    }
  }
  int nclassic = 0, ngeneral = 0;
  for (int k = 0; k < kJpegKinds; ++k) (k < kJpegGenKind ? nclassic : ngeneral) += L.count[k];
  std::vector<JpegImageDesc> id((size_t)nclassic);
  std::vector<JpegGenDesc> gd((size_t)ngeneral);
  if (!sc.coef.ensure(ncoef + 64, err) || !sc.planes.ensure(nplane + 256, err) || !sc.pd.ensure(pd.size(), err) || !sc.id.ensure(nclassic + 1, err) ||
      !sc.gd.ensure(ngeneral + 1, err))
    return OCR_ERR_DEVICE;
  const size_t coef_bytes = ncoef * sizeof(int16_t);
  if (!sc.stage.reserve(coef_bytes, err)) return OCR_ERR_DEVICE;
  {  // coefficient arrays -> pinned memory
    struct Piece { const int16_t* src; size_t off, n; };
    std::vector<Piece> pieces;
    size_t p = 0;
    for (int i = 0; i < count; ++i)
      for (int c = 0; c < imgs[i]->ncomp; ++c, ++p) pieces.push_back({imgs[i]->comp[c].coef, coef_off[p], (size_t)imgs[i]->comp[c].bw * imgs[i]->comp[c].bh * 64});
    int16_t* pinned = reinterpret_cast<int16_t*>(sc.stage.p);
    parallel_copy(pieces.size(), coef_bytes, [&](size_t k) { memcpy(pinned + pieces[k].off, pieces[k].src, pieces[k].n * sizeof(int16_t)); });
  }
  // image descriptors ordered by the kernel that writes them (the destination is in the descriptor: any order will do);
  // the kinds of before index `id`, the general kinds `gd`
  L.first[0] = 0;
  for (int k = 1; k < kJpegGenKind; ++k) L.first[k] = L.first[k - 1] + L.count[k - 1];
  L.first[kJpegGenKind] = 0;
  for (int k = kJpegGenKind + 1; k < kJpegKinds; ++k) L.first[k] = L.first[k - 1] + L.count[k - 1];
  int next[kJpegKinds];
  std::copy(L.first, L.first + kJpegKinds, next);
  size_t p = 0;
  for (int i = 0; i < count; ++i) {
    const ocr_jpeg_frame& im = *imgs[i];
    const int kind = kinds[i];
    const int orient = im.orientation ? im.orientation : 1;
    const FrameMax m = frame_max(im);
    L.blocks[kind] = std::max(L.blocks[kind], jpeg_output_blocks(im.rows, im.cols, orient));
    for (int c = 0; c < im.ncomp; ++c) {
      pd[p + c].coef = sc.coef.p + coef_off[p + c];
      pd[p + c].plane = sc.planes.p + plane_off[p + c];
    }
    if (kind < kJpegGenKind) {
      JpegImageDesc& d = id[next[kind]++];
      d = JpegImageDesc{};
      d.rows = im.rows; d.cols = im.cols; d.ncomp = im.ncomp; d.hmax = m.hmax; d.vmax = m.vmax; d.bgr = dst[i];
      d.orient = orient;
      for (int c = 0; c < im.ncomp; ++c) {
        d.plane[c] = pd[p + c].plane;
        d.stride[c] = im.comp[c].bw * 8;
        d.dw[c] = im.comp[c].dw;
        d.dh[c] = im.comp[c].dh;
      }
    } else {
      JpegGenDesc& d = gd[next[kind]++];
      d = JpegGenDesc{};
      d.rows = im.rows; d.cols = im.cols; d.ncomp = im.ncomp; d.color = im.color; d.bgr = dst[i];
      d.orient = orient;
      for (int c = 0; c < im.ncomp; ++c) {
        const ocr_jpeg_fcomp& k = im.comp[c];
        const int hexp = m.hmax / k.h, vexp = m.vmax / k.v;
        d.plane[c] = pd[p + c].plane;
        d.stride[c] = k.bw * 8;
        d.dw[c] = k.dw;
        d.dh[c] = k.dh;
        d.hexp[c] = (uint8_t)hexp;
        d.vexp[c] = (uint8_t)vexp;
        // jdsample.c: the fancy forms of 2x1 and 2x2 need a component more than 2 samples wide
        d.method[c] = (uint8_t)(hexp == 1 && vexp == 1 ? kJpegCopy : hexp == 2 && vexp == 1 ? (k.dw > 2 ? kJpegFancyH2V1 : kJpegBox)
                              : hexp == 1 && vexp == 2 ? kJpegFancyH1V2 : hexp == 2 && vexp == 2 ? (k.dw > 2 ? kJpegFancyH2V2 : kJpegBox) : kJpegBox);
      }
    }
    p += im.ncomp;
  }
  if (!sc.stage.upload(sc.coef.p, coef_bytes, s, err) ||
      hipMemcpyAsync(sc.pd.p, pd.data(), pd.size() * sizeof(JpegPlaneDesc), hipMemcpyHostToDevice, s) != hipSuccess ||
      (nclassic && hipMemcpyAsync(sc.id.p, id.data(), id.size() * sizeof(JpegImageDesc), hipMemcpyHostToDevice, s) != hipSuccess) ||
      (ngeneral && hipMemcpyAsync(sc.gd.p, gd.data(), gd.size() * sizeof(JpegGenDesc), hipMemcpyHostToDevice, s) != hipSuccess)) {
    err = "JPEG coefficient upload failed";
    return OCR_ERR_DEVICE;
  }
  L.ndesc = (int)pd.size();
  L.idct_blocks = nblocks;
  launch_jpeg_idct(sc.pd.p, L.ndesc, L.idct_blocks, s);
  launch_jpeg_output(sc.id.p, sc.gd.p, L, s);
  if (launched) *launched = L;
  if (hipGetLastError() != hipSuccess) { err = "JPEG kernels failed to launch"; return OCR_ERR_DEVICE; }
  return OCR_OK;
}

}  // namespace ocr

using namespace ocr;

namespace {

int decode_frame(const ocr_jpeg_frame& f, int device_id, uint8_t* bgr, size_t cap) {
  int rc = ocr_rt_init(device_id);
  if (rc) return rc;
  if (const char* fault = jpeg_frame_fault(f)) return fail(OCR_ERR_ARG, fault);
  const size_t bytes = (size_t)f.rows * f.cols * 3;
  if (bytes > cap) return fail(OCR_ERR_CAPACITY, "output buffer too small");
  JpegScratch sc;
  const ocr_jpeg_frame* frame = &f;
  return decode_one(bytes, bgr, [&](uint8_t* const* dst, std::string& err) { return jpeg_decode_async(&frame, 1, dst, sc, nullptr, err); });
}

int time_frame(const ocr_jpeg_frame& f, int device_id, int iters, double ms[2]) {
  int rc = ocr_rt_init(device_id);
  if (rc) return rc;
  if (const char* fault = jpeg_frame_fault(f)) return fail(OCR_ERR_ARG, fault);
  JpegScratch sc;
  DevBuf<uint8_t> out;
  std::string err;
  if (!out.ensure((size_t)f.rows * f.cols * 3, err)) return fail(OCR_ERR_DEVICE, err);
  uint8_t* dst = out.p;
  JpegLaunch L;
  const ocr_jpeg_frame* frame = &f;
  rc = jpeg_decode_async(&frame, 1, &dst, sc, nullptr, err, &L);  // uploads, and the first (untimed) launches
  if (rc) return fail(rc, err);
  return time_phases(iters, ms, [&] { launch_jpeg_idct(sc.pd.p, L.ndesc, L.idct_blocks, nullptr); return hipSuccess; },
                     [&] { launch_jpeg_output(sc.id.p, sc.gd.p, L, nullptr); return hipSuccess; });
}

}  // namespace

extern "C" int ocr_jpeg_decode(const ocr_jpeg_img* img, int device_id, uint8_t* bgr, size_t cap) {
  if (!img || !bgr) return fail(OCR_ERR_ARG, "null argument");
  int rc = ocr_rt_init(device_id);
  if (rc) return rc;
  if (!jpeg_img_valid(*img)) return fail(OCR_ERR_ARG, "bad JPEG coefficient descriptor");
  return decode_frame(jpeg_frame_of(*img), device_id, bgr, cap);
}

extern "C" int ocr_jpeg_time(const ocr_jpeg_img* img, int device_id, int iters, double ms[2]) {
  if (!img || !ms || iters <= 0) return fail(OCR_ERR_ARG, "null argument");
  int rc = ocr_rt_init(device_id);
  if (rc) return rc;
  if (!jpeg_img_valid(*img)) return fail(OCR_ERR_ARG, "bad JPEG coefficient descriptor");
  return time_frame(jpeg_frame_of(*img), device_id, iters, ms);
}

extern "C" int ocr_jpeg_decode_frame(const ocr_jpeg_frame* frame, int device_id, uint8_t* bgr, size_t cap) {
  if (!frame || !bgr) return fail(OCR_ERR_ARG, "null argument");
  return decode_frame(*frame, device_id, bgr, cap);
}

extern "C" int ocr_jpeg_time_frame(const ocr_jpeg_frame* frame, int device_id, int iters, double ms[2]) {
  if (!frame || !ms || iters <= 0) return fail(OCR_ERR_ARG, "null argument");
  return time_frame(*frame, device_id, iters, ms);
}
