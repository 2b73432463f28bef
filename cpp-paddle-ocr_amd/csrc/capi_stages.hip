// C-ABI: detector / classifier / recognizer handles (include/ocr_hip.h).
#include <cstring>
#include <memory>
#include <vector>

#include "capi_common.h"
#include "crop.h"
#include "rot_groups.h"
#include "stages.h"

using namespace ocr;

struct ocr_det { DetStage s; };
struct ocr_cls { ClsStage s; };
struct ocr_rec { RecStage s; };

extern "C" {

void ocr_det_cfg_default(ocr_det_cfg* c) {
  if (!c) return;
  memset(c, 0, sizeof(*c));
  // literals of OCRWorker::OCRWorker, /root/reference/src/ocr_worker.cpp:21-35
  c->model_dir = nullptr;
  c->device_id = 0;
  c->limit_type = "max";
  c->limit_side_len = 512;
  c->det_db_thresh = 0.2;
  c->det_db_box_thresh = 0.4;
  c->det_db_unclip_ratio = 1.8;
  c->det_db_score_mode = "fast";
  c->use_dilation = 0;
  c->precision = "fp32";
  c->max_batch = 1;
}

int ocr_det_create(const ocr_det_cfg* c, ocr_det** out) {
  if (!c || !out || !c->model_dir) return fail(OCR_ERR_ARG, "null argument");
  DetConfig cfg;
  cfg.model_dir = c->model_dir;
  cfg.device = c->device_id;
  if (c->limit_type) cfg.limit_type = c->limit_type;
  cfg.limit_side_len = c->limit_side_len;
  cfg.thresh = c->det_db_thresh;
  cfg.box_thresh = c->det_db_box_thresh;
  cfg.unclip_ratio = c->det_db_unclip_ratio;
  if (c->det_db_score_mode) cfg.score_mode = c->det_db_score_mode;
  cfg.use_dilation = c->use_dilation;
  if (c->precision) cfg.precision = c->precision;
  cfg.max_batch = c->max_batch > 0 ? c->max_batch : 1;
  cfg.cv_compat = resolve_cv_compat(c->cv_compat);
  std::unique_ptr<ocr_det> h(new ocr_det());
  std::string err;
  int code = 0;
  if (!h->s.create(cfg, err, code)) return fail(code, err);
  *out = h.release();
  return OCR_OK;
}
void ocr_det_destroy(ocr_det* h) { delete h; }

int ocr_det_run_batch(ocr_det* h, const ocr_img* imgs, int count, int32_t* boxes, int cap, int* n, double times[3]) {
  if (!h) return fail(OCR_ERR_ARG, "null handle");
  std::string err;
  const int rc = h->s.run(imgs, count, boxes, cap, n, times, err);
  return rc ? fail(rc, err) : OCR_OK;
}
int ocr_det_run(ocr_det* h, const ocr_img* img, int32_t* boxes, int cap, int* n, double times[3]) {
  return ocr_det_run_batch(h, img, 1, boxes, cap, n, times);
}
int ocr_det_last_shape(ocr_det* h, int* count, int* rows, int* cols) {
  if (!h) return fail(OCR_ERR_ARG, "null handle");
  if (count) *count = h->s.last_count;
  if (rows) *rows = h->s.last_h;
  if (cols) *cols = h->s.last_w;
  return OCR_OK;
}
static int det_tap(ocr_det* h, int index, const void* base, size_t elem, size_t per_px, void* out, size_t cap_elems) {
  if (!h || !out) return fail(OCR_ERR_ARG, "null argument");
  if (index < 0 || index >= h->s.last_count || !base) return fail(OCR_ERR_ARG, "no such image in the last run");
  const size_t cnt = (size_t)h->s.last_h * h->s.last_w * per_px;
  if (cnt > cap_elems) return fail(OCR_ERR_CAPACITY, "output buffer too small");
  CAPI_HIP(g_memcpy(out, (const char*)base + (size_t)index * cnt * elem, cnt * elem, hipMemcpyDeviceToHost));
  return OCR_OK;
}
int ocr_det_prob_map(ocr_det* h, int index, float* out, size_t cap) {
  return det_tap(h, index, h ? h->s.prob_dev() : nullptr, sizeof(float), 1, out, cap);
}
int ocr_det_bitmap(ocr_det* h, int index, uint8_t* out, size_t cap) {
  return det_tap(h, index, h ? h->s.bitmap_dev() : nullptr, 1, 1, out, cap);
}
int ocr_det_resized(ocr_det* h, int index, uint8_t* out, size_t cap) {
  return det_tap(h, index, h ? h->s.resized_dev() : nullptr, 1, 3, out, cap);
}
int ocr_det_post(ocr_det* h, const float* prob, int rows, int cols, int src_rows, int src_cols, int32_t* boxes, int cap,
                 int* n) {
  if (!h) return fail(OCR_ERR_ARG, "null handle");
  std::string err;
  const int rc = h->s.post_only(prob, rows, cols, src_rows, src_cols, boxes, cap, n, err);
  return rc ? fail(rc, err) : OCR_OK;
}

int ocr_det_post_stages(ocr_det* h, ocr_post_stages* out) {
  if (!h || !out) return fail(OCR_ERR_ARG, "null argument");
  std::string err;
  const int rc = h->s.post_stages(out, err);
  return rc ? fail(rc, err) : OCR_OK;
}

// ---- self-test taps: the device's ClipperOffset / UnClip in front of vectors the caller holds (tests/golden/unclip_ref*:
// outputs of the reference's own compiled src/clipper.cpp).  The calling thread's current device (ocr_rt_init).
int ocr_selftest_unclip(const int32_t* quads, const double* deltas, int n, int64_t* out, int cap, int* counts, double* trig) {
  if (!quads || !deltas || !out || !counts || n <= 0 || cap <= 0) return fail(OCR_ERR_ARG, "bad argument");
  int *dq = nullptr, *dc = nullptr;
  double *dd = nullptr, *dt = nullptr;
  if (trig) CAPI_HIP(g_malloc(&dt, (size_t)n * 3 * sizeof(double)));
  long long* dout = nullptr;
  CAPI_HIP(g_malloc(&dq, (size_t)n * 8 * sizeof(int)));
  CAPI_HIP(g_malloc(&dd, (size_t)n * sizeof(double)));
  CAPI_HIP(g_malloc(&dc, (size_t)n * sizeof(int)));
  CAPI_HIP(g_malloc(&dout, (size_t)n * cap * 2 * sizeof(long long)));
  CAPI_HIP(g_memcpy(dq, quads, (size_t)n * 8 * sizeof(int), hipMemcpyHostToDevice));
  CAPI_HIP(g_memcpy(dd, deltas, (size_t)n * sizeof(double), hipMemcpyHostToDevice));
  CAPI_HIP(hipMemset(dout, 0, (size_t)n * cap * 2 * sizeof(long long)));
  launch_selftest_clipper(dq, dd, n, dout, cap, dc, dt, nullptr);
  CAPI_HIP(hipGetLastError());
  if (trig) { CAPI_HIP(g_memcpy(trig, dt, (size_t)n * 3 * sizeof(double), hipMemcpyDeviceToHost)); (void)g_free(dt); }
  CAPI_HIP(g_memcpy(out, dout, (size_t)n * cap * 2 * sizeof(long long), hipMemcpyDeviceToHost));
  CAPI_HIP(g_memcpy(counts, dc, (size_t)n * sizeof(int), hipMemcpyDeviceToHost));
  (void)g_free(dq); (void)g_free(dd); (void)g_free(dc); (void)g_free(dout);
  return OCR_OK;
}
int ocr_selftest_unclip_box(const float* boxes, float unclip_ratio, int n, float* out14, int* status) {
  if (!boxes || !out14 || !status || n <= 0) return fail(OCR_ERR_ARG, "bad argument");
  float *db = nullptr, *dout = nullptr;
  int* dst = nullptr;
  CAPI_HIP(g_malloc(&db, (size_t)n * 8 * sizeof(float)));
  CAPI_HIP(g_malloc(&dout, (size_t)n * 14 * sizeof(float)));
  CAPI_HIP(g_malloc(&dst, (size_t)n * 2 * sizeof(int)));
  CAPI_HIP(g_memcpy(db, boxes, (size_t)n * 8 * sizeof(float), hipMemcpyHostToDevice));
  launch_selftest_unclip_box(db, unclip_ratio, n, dout, dst, nullptr);
  CAPI_HIP(hipGetLastError());
  CAPI_HIP(g_memcpy(out14, dout, (size_t)n * 14 * sizeof(float), hipMemcpyDeviceToHost));
  CAPI_HIP(g_memcpy(status, dst, (size_t)n * 2 * sizeof(int), hipMemcpyDeviceToHost));
  (void)g_free(db); (void)g_free(dout); (void)g_free(dst);
  return OCR_OK;
}

// ---- self-test taps: the resize-and-normalise launches of kernels_pre.hip alone.  Outputs are pre-filled with
// OCR_SELFTEST_FILL and handed back with OCR_SELFTEST_GUARD bytes from behind their last element; whatever the launchers
// leave undefined is refused here, before the device sees it.
namespace {
const int kPreMaxSide = 8192, kPreMaxCount = 1024;
const size_t kPreMaxBytes = (size_t)1 << 28;

bool upload_norm_lut(NormStage st, DevBuf<float>& lut, std::string& err) {
  const std::vector<float> h = stage_norm_lut(st);
  if (!lut.ensure(h.size(), err)) return false;
  if (g_memcpy(lut.p, h.data(), h.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) { err = "lut upload failed"; return false; }
  return true;
}
// the parent image and the ROIs (x, y, w, h, resize_w, .) of a line launch
const char* check_lines(const uint8_t* img, int rows, int cols, size_t stride, const int32_t* lines, int n, int imgH, int stage, const float* out) {
  if (!img || !lines || !out) return "null argument";
  if (rows < 1 || cols < 1 || rows > kPreMaxSide || cols > kPreMaxSide) return "parent image size out of range";
  if (stride < (size_t)cols * 3 || stride > (size_t)kPreMaxSide * 4) return "stride below 3 * cols";
  if (n < 1 || n > kPreMaxCount) return "line count out of range";
  if (imgH < 1 || imgH > kPreMaxSide) return "imgH out of range";
  if (stage != OCR_STAGE_REC && stage != OCR_STAGE_CLS) return "stage is neither OCR_STAGE_REC nor OCR_STAGE_CLS";
  for (int i = 0; i < n; ++i) {
    const int32_t* q = lines + (size_t)i * 6;
    if (q[2] < 1 || q[3] < 1) return "empty ROI";
    if (q[0] < 0 || q[1] < 0 || q[0] > cols - q[2] || q[1] > rows - q[3]) return "ROI outside the parent image";
    if (q[4] < 1) return "resize_w < 1";
  }
  return nullptr;
}
}  // namespace

int ocr_selftest_det_pre(const uint8_t* buf, size_t buf_bytes, size_t src_offset, size_t src_stride, size_t src_image_bytes, int N,
                         int sh, int sw, int dh, int dw, float* out, uint8_t* resized) {
  if (!buf || !out || !resized) return fail(OCR_ERR_ARG, "null argument");
  if (N < 1 || N > kPreMaxCount || sh < 1 || sw < 1 || dh < 1 || dw < 1 || sh > kPreMaxSide || sw > kPreMaxSide || dh > kPreMaxSide ||
      dw > kPreMaxSide)
    return fail(OCR_ERR_ARG, "image count or size out of range");
  if (buf_bytes < 1 || buf_bytes > kPreMaxBytes) return fail(OCR_ERR_ARG, "buffer size out of range");
  if (src_stride < (size_t)sw * 3 || src_stride > buf_bytes) return fail(OCR_ERR_ARG, "src_stride below 3 * sw");
  const size_t one = (size_t)(sh - 1) * src_stride + (size_t)sw * 3;  // bytes from an image's first to behind its last
  if (N > 1 && src_image_bytes < one) return fail(OCR_ERR_ARG, "src_image_bytes below the size of one image");
  if (src_image_bytes > buf_bytes || src_offset > buf_bytes || one > buf_bytes - src_offset ||
      (size_t)(N - 1) * src_image_bytes > buf_bytes - src_offset - one)
    return fail(OCR_ERR_ARG, "the images do not lie inside the buffer");
  const size_t nel = (size_t)N * dh * dw * 3;
  if (nel * sizeof(float) > kPreMaxBytes) return fail(OCR_ERR_ARG, "output too large");
  std::string err;
  DevBuf<uint8_t> dsrc, dres;
  DevBuf<float> dout, lut;
  const size_t out_bytes = nel * sizeof(float) + OCR_SELFTEST_GUARD, res_bytes = nel + OCR_SELFTEST_GUARD;
  if (!dsrc.ensure(buf_bytes, err) || !dres.ensure(res_bytes, err) || !dout.ensure(out_bytes / sizeof(float), err) ||
      !upload_norm_lut(NormStage::Det, lut, err))
    return fail(OCR_ERR_DEVICE, err);
  CAPI_HIP(g_memcpy(dsrc.p, buf, buf_bytes, hipMemcpyHostToDevice));
  CAPI_HIP(hipMemset(dout.p, OCR_SELFTEST_FILL, out_bytes));
  CAPI_HIP(hipMemset(dres.p, OCR_SELFTEST_FILL, res_bytes));
  DetPreArgs pa{};
  pa.src = dsrc.p + src_offset; pa.src_image_bytes = src_image_bytes; pa.src_stride = src_stride;
  pa.N = N; pa.sh = sh; pa.sw = sw; pa.dh = dh; pa.dw = dw; pa.lut = lut.p; pa.out = dout.p; pa.resized = dres.p;
  launch_det_pre(pa, nullptr);
  CAPI_HIP(hipGetLastError());
  CAPI_HIP(g_memcpy(out, dout.p, out_bytes, hipMemcpyDeviceToHost));
  CAPI_HIP(g_memcpy(resized, dres.p, res_bytes, hipMemcpyDeviceToHost));
  return OCR_OK;
}

int ocr_selftest_line_pre(const uint8_t* img, int rows, int cols, size_t stride, const int32_t* lines, int n, int imgH, int imgW,
                          int nslots, int pad_mode, int stage, float* out) {
  if (const char* why = check_lines(img, rows, cols, stride, lines, n, imgH, stage, out)) return fail(OCR_ERR_ARG, why);
  if (imgW < 1 || imgW > kPreMaxSide) return fail(OCR_ERR_ARG, "imgW out of range");
  if (pad_mode != OCR_PAD_REC && pad_mode != OCR_PAD_CLS) return fail(OCR_ERR_ARG, "pad_mode is neither OCR_PAD_REC nor OCR_PAD_CLS");
  if (nslots < n || nslots > kPreMaxCount) return fail(OCR_ERR_ARG, "fewer slots than lines");
  std::vector<char> taken(nslots, 0);
  for (int i = 0; i < n; ++i) {
    const int32_t* q = lines + (size_t)i * 6;
    if (q[4] > imgW) return fail(OCR_ERR_ARG, "resize_w above the tensor width");
    if (q[5] < 0 || q[5] >= nslots) return fail(OCR_ERR_ARG, "slot outside the tensor");
    if (taken[q[5]]) return fail(OCR_ERR_ARG, "two lines name one slot");
    taken[q[5]] = 1;
  }
  const size_t nel = (size_t)nslots * imgH * imgW * 3;
  if (nel * sizeof(float) > kPreMaxBytes) return fail(OCR_ERR_ARG, "output too large");
  std::string err;
  DevBuf<uint8_t> dimg;
  DevBuf<float> dout, lut;
  DevBuf<LineDesc> ddesc;
  const size_t out_bytes = nel * sizeof(float) + OCR_SELFTEST_GUARD;
  if (!dimg.ensure((size_t)rows * stride, err) || !dout.ensure(out_bytes / sizeof(float), err) || !ddesc.ensure(n, err) ||
      !upload_norm_lut(stage == OCR_STAGE_REC ? NormStage::Rec : NormStage::Cls, lut, err))
    return fail(OCR_ERR_DEVICE, err);
  std::vector<LineDesc> d(n);
  for (int i = 0; i < n; ++i) {
    const int32_t* q = lines + (size_t)i * 6;
    d[i] = LineDesc::make(dimg.p, stride, q[0], q[1], q[2], q[3], q[4], q[5], imgH);
  }
  CAPI_HIP(g_memcpy(dimg.p, img, (size_t)rows * stride, hipMemcpyHostToDevice));
  CAPI_HIP(g_memcpy(ddesc.p, d.data(), (size_t)n * sizeof(LineDesc), hipMemcpyHostToDevice));
  CAPI_HIP(hipMemset(dout.p, OCR_SELFTEST_FILL, out_bytes));
  launch_line_pre(ddesc.p, n, imgH, imgW, lut.p, pad_mode == OCR_PAD_CLS, dout.p, nullptr);
  CAPI_HIP(hipGetLastError());
  CAPI_HIP(g_memcpy(out, dout.p, out_bytes, hipMemcpyDeviceToHost));
  return OCR_OK;
}

int ocr_selftest_line_pre_ragged(const uint8_t* img, int rows, int cols, size_t stride, const int32_t* lines, int n, int imgH,
                                 int stage, float* out) {
  if (const char* why = check_lines(img, rows, cols, stride, lines, n, imgH, stage, out)) return fail(OCR_ERR_ARG, why);
  long pix = 0;
  for (int i = 0; i < n; ++i) {
    const int32_t* q = lines + (size_t)i * 6;
    if (q[5] < 1 || q[5] > kPreMaxSide) return fail(OCR_ERR_ARG, "tensor_w out of range");
    if (q[4] > q[5]) return fail(OCR_ERR_ARG, "resize_w above the tensor width");
    pix += (long)imgH * q[5];
  }
  const size_t nel = (size_t)pix * 3;
  if (nel * sizeof(float) > kPreMaxBytes) return fail(OCR_ERR_ARG, "output too large");
  std::string err;
  DevBuf<uint8_t> dimg;
  DevBuf<float> dout, lut;
  DevBuf<LineDesc> ddesc;
  const size_t out_bytes = nel * sizeof(float) + OCR_SELFTEST_GUARD;
  if (!dimg.ensure((size_t)rows * stride, err) || !dout.ensure(out_bytes / sizeof(float), err) || !ddesc.ensure(n, err) ||
      !upload_norm_lut(stage == OCR_STAGE_REC ? NormStage::Rec : NormStage::Cls, lut, err))
    return fail(OCR_ERR_DEVICE, err);
  std::vector<LineDesc> d(n);
  long at = 0;
  for (int i = 0; i < n; ++i) {
    const int32_t* q = lines + (size_t)i * 6;
    d[i] = LineDesc::make(dimg.p, stride, q[0], q[1], q[2], q[3], q[4], i, imgH);
    d[i].tensor_w = q[5];
    d[i].pix0 = (int)at;
    at += (long)imgH * q[5];
  }
  CAPI_HIP(g_memcpy(dimg.p, img, (size_t)rows * stride, hipMemcpyHostToDevice));
  CAPI_HIP(g_memcpy(ddesc.p, d.data(), (size_t)n * sizeof(LineDesc), hipMemcpyHostToDevice));
  CAPI_HIP(hipMemset(dout.p, OCR_SELFTEST_FILL, out_bytes));
  launch_line_pre_ragged(ddesc.p, n, pix, imgH, lut.p, dout.p, nullptr);
  CAPI_HIP(hipGetLastError());
  CAPI_HIP(g_memcpy(out, dout.p, out_bytes, hipMemcpyDeviceToHost));
  return OCR_OK;
}

// ---- self-test taps: the crop geometry between detector and recognizer alone (launch_warp_crops, launch_rotate180_groups,
// plan_rotate_crop, rot_groups::group).  The warp's matrix, column block and grid size and the rotation's segments are the
// caller's: the launches are checked where no box of the product leads.
int ocr_selftest_warp_crops(const uint8_t* src, size_t src_bytes, const ocr_warp_case* cases, int n, int max_pixels,
                            const uint64_t* out_off, size_t out_bytes, uint8_t* out) {
  if (!src || !cases || !out_off || !out) return fail(OCR_ERR_ARG, "null argument");
  if (n < 1 || n > kPreMaxCount) return fail(OCR_ERR_ARG, "crop count out of range");
  if (max_pixels < 1 || max_pixels > kPreMaxSide * kPreMaxSide) return fail(OCR_ERR_ARG, "max_pixels out of range");
  if (src_bytes < 1 || src_bytes > kPreMaxBytes || out_bytes < 1 || out_bytes > kPreMaxBytes) return fail(OCR_ERR_ARG, "buffer size out of range");
  for (int k = 0; k < n; ++k) {
    const ocr_warp_case& c = cases[k];
    if (c.sw < 1 || c.sh < 1 || c.dw < 1 || c.dh < 1 || c.sw > kPreMaxSide || c.sh > kPreMaxSide || c.dw > kPreMaxSide || c.dh > kPreMaxSide)
      return fail(OCR_ERR_ARG, "crop size out of range");
    if (c.bw0 < 1) return fail(OCR_ERR_ARG, "bw0 < 1");
    if (c.rot != 0 && c.rot != 1) return fail(OCR_ERR_ARG, "rot is neither 0 nor 1");
    if (c.sstride < (uint64_t)c.sw * 3 || c.sstride > src_bytes) return fail(OCR_ERR_ARG, "sstride below 3 * sw");
    const size_t one = (size_t)(c.sh - 1) * c.sstride + (size_t)c.sw * 3;
    if (c.src_off > src_bytes || one > src_bytes - c.src_off) return fail(OCR_ERR_ARG, "the source crop does not lie inside the buffer");
    const size_t bytes = (size_t)c.dw * c.dh * 3;
    if (out_off[k] > out_bytes || bytes > out_bytes - out_off[k]) return fail(OCR_ERR_ARG, "the crop does not lie inside the output");
  }
  std::string err;
  DevBuf<uint8_t> dsrc, dout;
  DevBuf<WarpDesc> ddesc;
  const size_t all = out_bytes + OCR_SELFTEST_GUARD;
  if (!dsrc.ensure(src_bytes, err) || !dout.ensure(all, err) || !ddesc.ensure(n, err)) return fail(OCR_ERR_DEVICE, err);
  std::vector<WarpDesc> wd(n);
  for (int k = 0; k < n; ++k) {
    const ocr_warp_case& c = cases[k];
    WarpDesc& d = wd[k];
    d.src = dsrc.p + c.src_off; d.sstride = c.sstride; d.sw = c.sw; d.sh = c.sh; d.dst = dout.p + out_off[k];
    d.dw = c.dw; d.dh = c.dh; d.rot = c.rot; d.bw0 = c.bw0;
    memcpy(d.m, c.m, sizeof(d.m));
  }
  CAPI_HIP(g_memcpy(dsrc.p, src, src_bytes, hipMemcpyHostToDevice));
  CAPI_HIP(g_memcpy(ddesc.p, wd.data(), (size_t)n * sizeof(WarpDesc), hipMemcpyHostToDevice));
  CAPI_HIP(hipMemset(dout.p, OCR_SELFTEST_FILL, all));
  launch_warp_crops(ddesc.p, n, max_pixels, nullptr);
  CAPI_HIP(hipGetLastError());
  CAPI_HIP(g_memcpy(out, dout.p, all, hipMemcpyDeviceToHost));
  return OCR_OK;
}

int ocr_selftest_rotate180_groups(uint8_t* buf, size_t buf_bytes, const int64_t* rois, int n, const int32_t* seg, int ngroups) {
  if (!buf || !rois || !seg) return fail(OCR_ERR_ARG, "null argument");
  if (n < 1 || n > kPreMaxCount) return fail(OCR_ERR_ARG, "ROI count out of range");
  if (ngroups < 0 || ngroups > n) return fail(OCR_ERR_ARG, "group count out of range");
  if (buf_bytes < 1 || buf_bytes > kPreMaxBytes) return fail(OCR_ERR_ARG, "buffer size out of range");
  if (seg[0] != 0) return fail(OCR_ERR_ARG, "seg[0] is not 0");
  for (int g = 0; g < ngroups; ++g)
    if (seg[g + 1] < seg[g] || seg[g + 1] > n) return fail(OCR_ERR_ARG, "seg is not ascending inside the ROI list");
  std::vector<size_t> first(n), last(n);  // the bytes an ROI's rotation may touch: [first, last)
  for (int k = 0; k < n; ++k) {
    const int64_t* q = rois + (size_t)k * 6;
    if (q[4] < 1 || q[5] < 1 || q[4] > kPreMaxSide || q[5] > kPreMaxSide) return fail(OCR_ERR_ARG, "empty ROI");
    if (q[2] < 0 || q[3] < 0 || q[2] > kPreMaxSide || q[3] > kPreMaxSide) return fail(OCR_ERR_ARG, "ROI origin out of range");
    if (q[0] < 0 || (uint64_t)q[0] > buf_bytes) return fail(OCR_ERR_ARG, "view outside the buffer");
    if (q[1] < (q[2] + q[4]) * 3 || (uint64_t)q[1] > buf_bytes) return fail(OCR_ERR_ARG, "stride below the ROI's right edge");
    first[k] = (size_t)q[0] + (size_t)q[3] * q[1] + (size_t)q[2] * 3;
    last[k] = (size_t)q[0] + (size_t)(q[3] + q[5] - 1) * q[1] + (size_t)(q[2] + q[4]) * 3;
    if (last[k] > buf_bytes) return fail(OCR_ERR_ARG, "ROI outside the buffer");
  }
  const int used = seg[ngroups];
  std::vector<int> group_of(used, 0);
  for (int g = 0; g < ngroups; ++g)
    for (int k = seg[g]; k < seg[g + 1]; ++k) group_of[k] = g;
  for (int a = 0; a < used; ++a)
    for (int b = a + 1; b < used; ++b) {
      if (group_of[a] == group_of[b]) continue;
      const int64_t *p = rois + (size_t)a * 6, *q = rois + (size_t)b * 6;
      const bool same_view = p[0] == q[0] && p[1] == q[1];
      const bool touch = same_view ? rot_groups::intersects(rot_groups::Rect{(int)p[2], (int)p[3], (int)p[4], (int)p[5]},
                                                            rot_groups::Rect{(int)q[2], (int)q[3], (int)q[4], (int)q[5]})
                                   : first[a] < last[b] && first[b] < last[a];
      if (touch) return fail(OCR_ERR_ARG, "ROIs of two groups may touch the same bytes");
    }
  std::string err;
  DevBuf<uint8_t> dimg;
  DevBuf<RotDesc> ddesc;
  DevBuf<int> dseg;
  if (!dimg.ensure(buf_bytes, err) || !ddesc.ensure(n, err) || !dseg.ensure((size_t)ngroups + 1, err)) return fail(OCR_ERR_DEVICE, err);
  std::vector<RotDesc> rd(n);
  for (int k = 0; k < n; ++k) {
    const int64_t* q = rois + (size_t)k * 6;
    rd[k] = RotDesc{dimg.p + q[0], (size_t)q[1], (int)q[2], (int)q[3], (int)q[4], (int)q[5]};
  }
  CAPI_HIP(g_memcpy(dimg.p, buf, buf_bytes, hipMemcpyHostToDevice));
  CAPI_HIP(g_memcpy(ddesc.p, rd.data(), (size_t)n * sizeof(RotDesc), hipMemcpyHostToDevice));
  CAPI_HIP(g_memcpy(dseg.p, seg, ((size_t)ngroups + 1) * sizeof(int), hipMemcpyHostToDevice));
  launch_rotate180_groups(ddesc.p, dseg.p, ngroups, nullptr);
  CAPI_HIP(hipGetLastError());
  CAPI_HIP(g_memcpy(buf, dimg.p, buf_bytes, hipMemcpyDeviceToHost));
  return OCR_OK;
}

int ocr_selftest_crop_plan(int rows, int cols, const int32_t* box8, int32_t* fields, double* minv) {
  if (!box8 || !fields || !minv) return fail(OCR_ERR_ARG, "null argument");
  CropPlan p;
  if (!plan_rotate_crop(rows, cols, box8, p)) return fail(OCR_ERR_ARG, "box has no crop inside the image");
  const int32_t f[10] = {p.left, p.top, p.sw, p.sh, p.dw, p.dh, p.rot, p.orows, p.ocols, p.bw0};
  memcpy(fields, f, sizeof(f));
  memcpy(minv, p.minv, sizeof(p.minv));
  return OCR_OK;
}

int ocr_selftest_rotation_groups(const int32_t* rects, const int32_t* views, int n, int32_t* order, int32_t* seg, int* ngroups) {
  if (!rects || !views || !order || !seg || !ngroups) return fail(OCR_ERR_ARG, "null argument");
  if (n < 1 || n > (1 << 20)) return fail(OCR_ERR_ARG, "rectangle count out of range");
  std::vector<rot_groups::Rect> r(n);
  std::vector<int32_t> v(views, views + n);
  for (int k = 0; k < n; ++k) {
    const int32_t* q = rects + (size_t)k * 4;
    if (q[2] < 1 || q[3] < 1 || q[0] > INT32_MAX - q[2] || q[1] > INT32_MAX - q[3]) return fail(OCR_ERR_ARG, "empty rectangle");
    r[k] = rot_groups::Rect{q[0], q[1], q[2], q[3]};
  }
  std::vector<int> ord, sg;
  rot_groups::group(r, v, ord, sg);
  for (int k = 0; k < n; ++k) order[k] = ord[k];
  for (size_t g = 0; g < sg.size(); ++g) seg[g] = sg[g];
  *ngroups = (int)sg.size() - 1;
  return OCR_OK;
}

void ocr_cls_cfg_default(ocr_cls_cfg* c) {
  if (!c) return;
  memset(c, 0, sizeof(*c));
  c->cls_thresh = 0.98;   // ocr_worker.cpp:45
  c->cls_batch_num = 8;   // ocr_worker.cpp:47
  c->precision = "fp32";
}
int ocr_cls_create(const ocr_cls_cfg* c, ocr_cls** out) {
  if (!c || !out || !c->model_dir) return fail(OCR_ERR_ARG, "null argument");
  ClsConfig cfg;
  cfg.model_dir = c->model_dir;
  cfg.device = c->device_id;
  cfg.thresh = c->cls_thresh;
  cfg.batch_num = c->cls_batch_num > 0 ? c->cls_batch_num : 1;
  if (c->precision) cfg.precision = c->precision;
  std::unique_ptr<ocr_cls> h(new ocr_cls());
  std::string err;
  int code = 0;
  if (!h->s.create(cfg, err, code)) return fail(code, err);
  *out = h.release();
  return OCR_OK;
}
void ocr_cls_destroy(ocr_cls* h) { delete h; }
int ocr_cls_run(ocr_cls* h, const ocr_img* imgs, int n, int* labels, float* scores, double times[3]) {
  if (!h) return fail(OCR_ERR_ARG, "null handle");
  std::string err;
  const int rc = h->s.run(imgs, n, labels, scores, times, err);
  return rc ? fail(rc, err) : OCR_OK;
}
int ocr_cls_probs(ocr_cls* h, float* out, size_t cap) {
  if (!h || !out) return fail(OCR_ERR_ARG, "null argument");
  if (h->s.tap_probs.size() > cap) return fail(OCR_ERR_CAPACITY, "output buffer too small");
  memcpy(out, h->s.tap_probs.data(), h->s.tap_probs.size() * sizeof(float));
  return OCR_OK;
}

void ocr_rec_cfg_default(ocr_rec_cfg* c) {
  if (!c) return;
  memset(c, 0, sizeof(*c));
  c->rec_batch_num = 16;  // ocr_worker.cpp:60-62
  c->rec_img_h = 28;
  c->rec_img_w = 192;
  c->precision = "fp32";
}
int ocr_rec_create(const ocr_rec_cfg* c, ocr_rec** out) {
  if (!c || !out || !c->model_dir || !c->label_path) return fail(OCR_ERR_ARG, "null argument");
  RecConfig cfg;
  cfg.model_dir = c->model_dir;
  cfg.label_path = c->label_path;
  cfg.device = c->device_id;
  cfg.batch_num = c->rec_batch_num;
  cfg.sort_mode = c->sort_mode;
  cfg.img_h = c->rec_img_h;
  cfg.img_w = c->rec_img_w;
  if (c->precision) cfg.precision = c->precision;
  std::unique_ptr<ocr_rec> h(new ocr_rec());
  std::string err;
  int code = 0;
  if (!h->s.create(cfg, err, code)) return fail(code, err);
  *out = h.release();
  return OCR_OK;
}
void ocr_rec_destroy(ocr_rec* h) { delete h; }
int ocr_rec_run(ocr_rec* h, const ocr_img* imgs, int n, int32_t* ids, int max_len, int* lens, float* scores,
                double times[3]) {
  if (!h) return fail(OCR_ERR_ARG, "null handle");
  std::string err;
  const int rc = h->s.run(imgs, n, ids, max_len, lens, scores, times, err);
  return rc ? fail(rc, err) : OCR_OK;
}
int ocr_rec_run_chars(ocr_rec* h, const ocr_img* imgs, int n, int32_t* ids, int max_len, int* lens, float* scores, int32_t* steps,
                      int32_t* nsteps, float* probs, int32_t* geom, int topk, int32_t* alt_ids, float* alt_probs, double times[3]) {
  if (!h) return fail(OCR_ERR_ARG, "null handle");
  RecStage::CharOut co;
  co.steps = steps; co.nsteps = nsteps; co.probs = probs; co.geom = geom;
  co.topk = topk; co.alt_ids = alt_ids; co.alt_probs = alt_probs;
  std::string err;
  const int rc = h->s.run_chars(imgs, n, ids, max_len, lens, scores, co, times, err);
  return rc ? fail(rc, err) : OCR_OK;
}
int ocr_rec_logits_row(ocr_rec* h, int index, int step, float* out, size_t cap_floats) {
  if (!h) return fail(OCR_ERR_ARG, "null handle");
  std::string err;
  const int rc = h->s.logits_row(index, step, out, cap_floats, err);
  return rc ? fail(rc, err) : OCR_OK;
}
// self-test: the top-k kernel alone - every caller row is "line i, one step, one kept character" of a uniform table
int ocr_selftest_topk(const float* rows, int n, int C, int pitch, const float* p0, int k, int32_t* out_ids, float* out_probs) {
  if (!rows || !p0 || !out_ids || !out_probs || n < 1 || C < 1 || pitch < C || k < 1 || k > 8) return fail(OCR_ERR_ARG, "bad argument");
  std::string err;
  DevBuf<float> drows, dp0, dprobs;
  DevBuf<int> dlens, dsteps, dids;
  const size_t nfl = (size_t)(n - 1) * pitch + C;
  if (!drows.ensure(nfl, err) || !dp0.ensure(n, err) || !dprobs.ensure((size_t)n * k, err) || !dlens.ensure(n, err) ||
      !dsteps.ensure(n, err) || !dids.ensure((size_t)n * k, err))
    return fail(OCR_ERR_DEVICE, err);
  const std::vector<int> ones(n, 1), zeros(n, 0);
  CAPI_HIP(g_memcpy(drows.p, rows, nfl * sizeof(float), hipMemcpyHostToDevice));
  CAPI_HIP(g_memcpy(dp0.p, p0, (size_t)n * sizeof(float), hipMemcpyHostToDevice));
  CAPI_HIP(g_memcpy(dlens.p, ones.data(), (size_t)n * sizeof(int), hipMemcpyHostToDevice));
  CAPI_HIP(g_memcpy(dsteps.p, zeros.data(), (size_t)n * sizeof(int), hipMemcpyHostToDevice));
  launch_ctc_topk(drows.p, pitch, C, k, nullptr, n, 1, 1, dlens.p, dsteps.p, dp0.p, dids.p, dprobs.p, nullptr);
  CAPI_HIP(hipGetLastError());
  CAPI_HIP(g_memcpy(out_ids, dids.p, (size_t)n * k * sizeof(int), hipMemcpyDeviceToHost));
  CAPI_HIP(g_memcpy(out_probs, dprobs.p, (size_t)n * k * sizeof(float), hipMemcpyDeviceToHost));
  return OCR_OK;
}
// ---- self-test taps: the recognizer's tail launches alone (tests/test_gpu_rec_tail.py).  Outputs pre-filled with
// OCR_SELFTEST_FILL, each handed back with OCR_SELFTEST_GUARD bytes from behind its last element.
extern "C++" {
namespace {
const long kTailMaxRows = 1 << 20, kTailMaxLines = 1 << 18;
const int kTailMaxSteps = 4096, kTailMaxLen = 4096;
const size_t kTailMaxBytes = (size_t)1 << 28;

// a pre-filled device array of n elements + guard
template <typename T>
bool tail_out(DevBuf<uint8_t>& d, size_t n, std::string& err) {
  const size_t bytes = n * sizeof(T) + OCR_SELFTEST_GUARD;
  if (!d.ensure(bytes, err)) return false;
  if (hipMemset(d.p, OCR_SELFTEST_FILL, bytes) != hipSuccess) { err = "hipMemset failed"; return false; }
  return true;
}
template <typename T>
hipError_t tail_back(void* host, const DevBuf<uint8_t>& d, size_t n) {
  return g_memcpy(host, d.p, n * sizeof(T) + OCR_SELFTEST_GUARD, hipMemcpyDeviceToHost);
}
template <typename T>
bool tail_in(DevBuf<T>& d, const T* host, size_t n, std::string& err) {
  if (!d.ensure(n, err)) return false;
  if (g_memcpy(d.p, host, n * sizeof(T), hipMemcpyHostToDevice) != hipSuccess) { err = "upload failed"; return false; }
  return true;
}
}  // namespace
}  // extern "C++"

int ocr_selftest_topk_lines(const float* rows, int nlines, int T, int C, int pitch, const int32_t* lens, const int32_t* steps,
                            const float* p0, int max_len, int k, int32_t* out_ids, float* out_probs) {
  if (!rows || !lens || !steps || !p0 || !out_ids || !out_probs) return fail(OCR_ERR_ARG, "null argument");
  if (nlines < 1 || nlines > kTailMaxLines || T < 1 || T > kTailMaxSteps || C < 1 || pitch < C || k < 1 || k > 8 || max_len < 1 ||
      max_len > kTailMaxLen)
    return fail(OCR_ERR_ARG, "size out of range");
  const size_t nrows = (size_t)nlines * T, nfl = (nrows - 1) * pitch + C, nch = (size_t)nlines * max_len;
  if (nfl * sizeof(float) > kTailMaxBytes || nch * k * sizeof(float) > kTailMaxBytes) return fail(OCR_ERR_ARG, "buffers too large");
  for (int i = 0; i < nlines; ++i) {
    if (lens[i] < 0) return fail(OCR_ERR_ARG, "negative line length");
    for (int j = 0; j < std::min(lens[i], max_len); ++j)
      if (steps[(size_t)i * max_len + j] < 0 || steps[(size_t)i * max_len + j] >= T) return fail(OCR_ERR_ARG, "step outside the line");
  }
  std::string err;
  DevBuf<float> drows, dp0;
  DevBuf<int> dlens, dsteps;
  DevBuf<uint8_t> dids, dprobs;
  if (!tail_in(drows, rows, nfl, err) || !tail_in(dp0, p0, nch, err) || !tail_in(dlens, (const int*)lens, (size_t)nlines, err) ||
      !tail_in(dsteps, (const int*)steps, nch, err) || !tail_out<int>(dids, nch * k, err) || !tail_out<float>(dprobs, nch * k, err))
    return fail(OCR_ERR_DEVICE, err);
  launch_ctc_topk(drows.p, pitch, C, k, nullptr, nlines, T, max_len, dlens.p, dsteps.p, dp0.p, (int*)dids.p, (float*)dprobs.p, nullptr);
  CAPI_HIP(hipGetLastError());
  CAPI_HIP(tail_back<int>(out_ids, dids, nch * k));
  CAPI_HIP(tail_back<float>(out_probs, dprobs, nch * k));
  return OCR_OK;
}

int ocr_selftest_softmax_argmax(const float* logits, long rows, int C, float* probs, int32_t* amax, float* pmax) {
  if (!logits || !amax || !pmax) return fail(OCR_ERR_ARG, "null argument");
  if (rows < 1 || rows > kTailMaxRows || C < 1) return fail(OCR_ERR_ARG, "rows or columns out of range");
  if (C > kSoftmaxMaxCols) return fail(OCR_ERR_ARG, "more columns than softmax_argmax_kernel takes (8192)");
  const size_t nel = (size_t)rows * C;
  if (nel * sizeof(float) > kTailMaxBytes) return fail(OCR_ERR_ARG, "logits too large");
  std::string err;
  DevBuf<float> dx;
  DevBuf<uint8_t> dq, da, dp;
  if (!tail_in(dx, logits, nel, err) || (probs && !tail_out<float>(dq, nel, err)) || !tail_out<int>(da, (size_t)rows, err) ||
      !tail_out<float>(dp, (size_t)rows, err))
    return fail(OCR_ERR_DEVICE, err);
  launch_softmax_argmax(dx.p, probs ? (float*)dq.p : nullptr, (int*)da.p, (float*)dp.p, rows, C, nullptr);
  CAPI_HIP(hipGetLastError());
  if (probs) CAPI_HIP(tail_back<float>(probs, dq, nel));
  CAPI_HIP(tail_back<int>(amax, da, (size_t)rows));
  CAPI_HIP(tail_back<float>(pmax, dp, (size_t)rows));
  return OCR_OK;
}

int ocr_selftest_head_combine(const float* hmax, const float* hsum, const int32_t* hidx, long rows, int groups, int32_t* amax,
                              float* pmax) {
  if (!hmax || !hsum || !hidx || !amax || !pmax) return fail(OCR_ERR_ARG, "null argument");
  if (rows < 1 || rows > kTailMaxRows || groups < 1 || groups > 1 << 16) return fail(OCR_ERR_ARG, "rows or groups out of range");
  const size_t nel = (size_t)rows * groups;
  if (nel * sizeof(float) > kTailMaxBytes) return fail(OCR_ERR_ARG, "partials too large");
  std::string err;
  DevBuf<float> dm, ds;
  DevBuf<int> di;
  DevBuf<uint8_t> da, dp;
  if (!tail_in(dm, hmax, nel, err) || !tail_in(ds, hsum, nel, err) || !tail_in(di, (const int*)hidx, nel, err) ||
      !tail_out<int>(da, (size_t)rows, err) || !tail_out<float>(dp, (size_t)rows, err))
    return fail(OCR_ERR_DEVICE, err);
  launch_head_combine(dm.p, ds.p, di.p, rows, groups, (int*)da.p, (float*)dp.p, nullptr);
  CAPI_HIP(hipGetLastError());
  CAPI_HIP(tail_back<int>(amax, da, (size_t)rows));
  CAPI_HIP(tail_back<float>(pmax, dp, (size_t)rows));
  return OCR_OK;
}

int ocr_selftest_ctc(const int32_t* amax, const float* pmax, long nsteps_total, int nlines, int T, const int32_t* lines, int max_len,
                     int chars, int32_t* ids, int32_t* lens, float* scores, int32_t* steps, int32_t* nsteps, float* probs) {
  if (!amax || !pmax || !ids || !lens || !scores) return fail(OCR_ERR_ARG, "null argument");
  if (chars && (!steps || !nsteps || !probs)) return fail(OCR_ERR_ARG, "null argument (per-character outputs)");
  if (nlines < 1 || nlines > kTailMaxLines || max_len < 1 || max_len > kTailMaxLen) return fail(OCR_ERR_ARG, "line count or max_len out of range");
  if (nsteps_total < 1 || nsteps_total > kTailMaxRows) return fail(OCR_ERR_ARG, "step count out of range");
  if (lines) {
    for (int i = 0; i < nlines; ++i) {
      const int32_t s0 = lines[2 * i], n = lines[2 * i + 1];
      if (n < 0 || n > kTailMaxSteps || s0 < 0 || s0 > nsteps_total - n) return fail(OCR_ERR_ARG, "a line's steps lie outside the step arrays");
    }
  } else if (T < 1 || T > kTailMaxSteps || (long)nlines * T != nsteps_total) {
    return fail(OCR_ERR_ARG, "T out of range or nlines * T is not the step count");
  }
  const size_t nch = (size_t)nlines * max_len;
  std::string err;
  DevBuf<int> dam;
  DevBuf<float> dpm;
  DevBuf<LineDesc> ddesc;
  DevBuf<uint8_t> dids, dlens, dsc, dst, dns, dpr;
  if (!tail_in(dam, (const int*)amax, (size_t)nsteps_total, err) || !tail_in(dpm, pmax, (size_t)nsteps_total, err) ||
      !tail_out<int>(dids, nch, err) || !tail_out<int>(dlens, (size_t)nlines, err) || !tail_out<float>(dsc, (size_t)nlines, err))
    return fail(OCR_ERR_DEVICE, err);
  if (chars && (!tail_out<int>(dst, nch, err) || !tail_out<int>(dns, nch, err) || !tail_out<float>(dpr, nch, err))) return fail(OCR_ERR_DEVICE, err);
  if (lines) {
    std::vector<LineDesc> d((size_t)nlines, LineDesc::make(nullptr, 0, 0, 0, 1, 1, 1, 0, 1));
    for (int i = 0; i < nlines; ++i) { d[i].slot = i; d[i].step0 = lines[2 * i]; d[i].steps = lines[2 * i + 1]; }
    if (!tail_in(ddesc, (const LineDesc*)d.data(), (size_t)nlines, err)) return fail(OCR_ERR_DEVICE, err);
  }
  if (chars)
    launch_ctc_chars(dam.p, dpm.p, lines ? ddesc.p : nullptr, nlines, T, max_len, (int*)dids.p, (int*)dlens.p, (float*)dsc.p, (int*)dst.p,
                     (int*)dns.p, (float*)dpr.p, nullptr);
  else if (lines)
    launch_ctc_ragged(dam.p, dpm.p, ddesc.p, nlines, max_len, (int*)dids.p, (int*)dlens.p, (float*)dsc.p, nullptr);
  else
    launch_ctc(dam.p, dpm.p, nlines, T, max_len, (int*)dids.p, (int*)dlens.p, (float*)dsc.p, nullptr);
  CAPI_HIP(hipGetLastError());
  CAPI_HIP(tail_back<int>(ids, dids, nch));
  CAPI_HIP(tail_back<int>(lens, dlens, (size_t)nlines));
  CAPI_HIP(tail_back<float>(scores, dsc, (size_t)nlines));
  if (chars) {
    CAPI_HIP(tail_back<int>(steps, dst, nch));
    CAPI_HIP(tail_back<int>(nsteps, dns, nch));
    CAPI_HIP(tail_back<float>(probs, dpr, nch));
  }
  return OCR_OK;
}

int ocr_selftest_srv_argmax(const float* logits, long rows, int C, int ld, int one_pass, int32_t* amax, float* pmax) {
  if (!logits || !amax || !pmax) return fail(OCR_ERR_ARG, "null argument");
  if (rows < 1 || rows > kTailMaxRows || C < 1 || ld < C) return fail(OCR_ERR_ARG, "rows, columns or row pitch out of range");
  if (one_pass && (ld % 4 != 0 || ld < ((C + 3) & ~3))) return fail(OCR_ERR_ARG, "the one-pass form reads 16 bytes at a time: ld % 4 == 0 and ld >= C rounded up to 4");
  const size_t nel = (size_t)rows * ld;  // (whole rows: the one-pass form reads up to the row's pitch)
  if (nel * sizeof(float) > kTailMaxBytes) return fail(OCR_ERR_ARG, "logits too large");
  std::string err;
  DevBuf<float> dx;
  DevBuf<uint8_t> da, dp;
  if (!tail_in(dx, logits, nel, err) || !tail_out<int>(da, (size_t)rows, err) || !tail_out<float>(dp, (size_t)rows, err))
    return fail(OCR_ERR_DEVICE, err);
  srv::launch_argmax_softmax(dx.p, rows, C, ld, (int*)da.p, (float*)dp.p, one_pass != 0, nullptr);
  CAPI_HIP(hipGetLastError());
  CAPI_HIP(tail_back<int>(amax, da, (size_t)rows));
  CAPI_HIP(tail_back<float>(pmax, dp, (size_t)rows));
  return OCR_OK;
}

int ocr_selftest_ctc_reduce(const float* part, long rows, int slots, int step, int32_t* amax, float* pmax) {
  if (!part || !amax || !pmax) return fail(OCR_ERR_ARG, "null argument");
  if (rows < 1 || rows > kTailMaxRows || slots < 1 || slots > 1 << 16 || step < 1 || step > slots) return fail(OCR_ERR_ARG, "rows, slots or step out of range");
  const size_t nel = (size_t)rows * slots * 4;
  if (nel * sizeof(float) > kTailMaxBytes) return fail(OCR_ERR_ARG, "partials too large");
  std::string err;
  DevBuf<float> dx;
  DevBuf<uint8_t> da, dp;
  if (!tail_in(dx, part, nel, err) || !tail_out<int>(da, (size_t)rows, err) || !tail_out<float>(dp, (size_t)rows, err))
    return fail(OCR_ERR_DEVICE, err);
  srv::launch_ctc_reduce(dx.p, rows, slots, step, (int*)da.p, (float*)dp.p, nullptr);
  CAPI_HIP(hipGetLastError());
  CAPI_HIP(tail_back<int>(amax, da, (size_t)rows));
  CAPI_HIP(tail_back<float>(pmax, dp, (size_t)rows));
  return OCR_OK;
}

const char* ocr_rec_label(ocr_rec* h, int id) {
  if (!h || id < 0 || id >= (int)h->s.labels().size()) return nullptr;
  return h->s.labels()[id].c_str();
}
int ocr_rec_num_classes(ocr_rec* h) { return h ? (int)h->s.labels().size() : 0; }
int ocr_rec_steps(ocr_rec* h, int index, int32_t* amax, float* pmax, int cap, int* T) {
  if (!h || !T) return fail(OCR_ERR_ARG, "null argument");
  if (index < 0 || index >= (int)h->s.tap_T.size()) return fail(OCR_ERR_ARG, "no such line in the last run");
  const int t = h->s.tap_T[index];
  *T = t;
  if (t > cap) return fail(OCR_ERR_CAPACITY, "output buffer too small");
  if (amax) memcpy(amax, h->s.tap_amax.data() + h->s.tap_off[index], t * sizeof(int));
  if (pmax) memcpy(pmax, h->s.tap_pmax.data() + h->s.tap_off[index], t * sizeof(float));
  return OCR_OK;
}
int ocr_rec_set_launch_lines(ocr_rec* h, int n) {
  if (!h) return fail(OCR_ERR_ARG, "null handle");
  if (n < 1) return fail(OCR_ERR_ARG, "lines per launch must be >= 1");
  h->s.max_lines_per_launch = n;
  return OCR_OK;
}
int ocr_rec_timing(ocr_rec* h, int enable) {
  if (!h) return fail(OCR_ERR_ARG, "null handle");
  SrvNet* srv = h->s.srv();
  if (!srv) return fail(OCR_ERR_ARG, "launch timing of a recognizer handle: the server recognizer only");
  srv->enable_timing(enable != 0);
  srv->reset_timings();
  return OCR_OK;
}
int ocr_rec_timing_report(ocr_rec* h, char* buf, size_t cap) {
  if (!h || !buf) return fail(OCR_ERR_ARG, "null argument");
  SrvNet* srv = h->s.srv();
  if (!srv) return fail(OCR_ERR_ARG, "launch timing of a recognizer handle: the server recognizer only");
  size_t off = 0;
  for (auto& kv : srv->timings()) {
    int n = snprintf(buf + off, cap > off ? cap - off : 0, "%s %.6f %ld %.0f %.0f\n", kv.first.c_str(), kv.second.ms, kv.second.count,
                     kv.second.flops, kv.second.bytes);
    if (n < 0 || off + n >= cap) return fail(OCR_ERR_CAPACITY, "report buffer too small");
    off += n;
  }
  if (off < cap) buf[off] = 0;
  return OCR_OK;
}

}  // extern "C"
