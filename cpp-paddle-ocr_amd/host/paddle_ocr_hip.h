// Host layer above the C-ABI (include/ocr_hip.h): the reference's operator interface for this path
// with the same names, argument meaning and error behaviour, over an ImageView instead of cv::Mat.
//
//   PaddleOCR::DBDetector      /root/reference/include/paddle_ocr/ocr_det.h:28-131
//   PaddleOCR::Classifier      /root/reference/include/paddle_ocr/ocr_cls.h:28-104
//   PaddleOCR::CRNNRecognizer  /root/reference/include/paddle_ocr/ocr_rec.h:28-122
//   PaddleOCR::OCRRequest / WordResult / OCRResult / OCRWorker   include/paddle_ocr/ocr_worker.h:22-94
//   PaddleOCR::GPUWorkerPool   include/paddle_ocr/gpu_worker_pool.h:14-31
//
// Differences, all forced by the missing third-party types: images are `ImageView` (the fields of a
// CV_8UC3 cv::Mat that the path reads); the worker's result is an OCRResult plus a JSON string with
// the reference's keys (src/ocr_worker.cpp:155-190) written by a 40-line emitter instead of jsoncpp.
// Header-only; link with -locr_hip.
#pragma once
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <future>
#include <memory>
#include <mutex>
#include <queue>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

#include "../../include/ocr_hip.h"
#include "jpeg_decode.h"
#include "png_decode.h"
#include "raw_decode.h"
#include "tiff_decode.h"
#include "webp_decode.h"
#include "vp8_decode.h"
#include "j2k_decode.h"

namespace PaddleOCR {

// The part of cv::Mat this path uses: CV_8UC3 BGR rows, possibly an ROI of a larger image.
struct ImageView {
  const uint8_t* data = nullptr;
  int rows = 0, cols = 0;
  size_t step = 0;  // bytes per row
  bool empty() const { return !data || rows <= 0 || cols <= 0; }
  ImageView roi(int x, int y, int w, int h) const { return ImageView{data + (size_t)y * step + (size_t)x * 3, h, w, step}; }
  ocr_img c() const { return ocr_img{data, rows, cols, step}; }
};

// An owning image (cv::Mat::clone()).
struct Image {
  std::vector<uint8_t> pixels;
  int rows = 0, cols = 0;
  // a JPEG that has only been entropy-decoded: the worker finishes it on the device (ocr_pipe_stage_frames); `pixels`
  // stays empty unless someone asks for them (materialise()).  rows / cols are the size after the EXIF orientation, the
  // frame of the reply's width, height and boxes (cv::imdecode turns the image); jpeg->rows / cols stay the stored size
  std::shared_ptr<jpeg::Coefs> jpeg;
  // a PNG that has only been parsed and inflated: the worker unfilters and converts it on the device (ocr_pipe_stage_frames)
  std::shared_ptr<png::Frame> png;
  // a BMP / PNM whose container has been parsed (and run-length stream or ASCII numbers expanded): the worker converts the
  // stored rows on the device (ocr_pipe_stage_frames)
  std::shared_ptr<raw::Frame> raw;
  // a TIFF whose container has been parsed and whose chunks have been expanded (PackBits / LZW / Deflate): the worker undoes
  // the predictor, converts and places the chunks on the device (ocr_pipe_stage_batch)
  std::shared_ptr<tiff::Frame> tiff;
  // a TIFF whose container alone has been parsed (Compression 1, LZW, PackBits): the worker expands the chunks on the device
  // as well, then goes on as for tiff (ocr_pipe_stage_batch, OCR_FRAME_TIFF_CODED)
  std::shared_ptr<tiff::Coded> tiff_coded;
  // a Deflate TIFF whose container alone has been parsed (tiff::parse_deflate; no stream has been looked at): the worker
  // inflates the chunks on the device and refuses the batch where a stream falls short (ocr_pipe_stage_batch,
  // OCR_FRAME_TIFF_DEFLATE).  materialise() is the host's verdict on the same bytes (tiff::inflate_all) and THROWS where a
  // stream is faulty - of all kinds this one alone can, the others were checked before they got here - so the worker calls it
  // per request and fails that request alone; where the device refused, the worker asks it and the host's answer stands
  std::shared_ptr<tiff::Coded> tiff_deflate;
  // a CCITT fax TIFF whose container alone has been parsed and whose streams have been walked (tiff::parse_fax): the worker
  // expands the chunks on the device, then goes on as for tiff (ocr_pipe_stage_batch, OCR_FRAME_TIFF_FAX)
  std::shared_ptr<tiff::Coded> tiff_fax;
  // a lossless WebP whose entropy-coded image has been decoded (prefix codes, LZ77, colour cache): the worker undoes the
  // transforms on the device (ocr_pipe_stage_batch)
  std::shared_ptr<webp::Frame> webp;
  // a lossy WebP whose key frame has been parsed (boolean decoder, modes, tokens): the worker reconstructs, filters and
  // converts on the device (ocr_pipe_stage_batch)
  std::shared_ptr<vp8::Frame> vp8;
  // a JPEG 2000 file after tier-1 (boxes, markers, packet headers, MQ decoding): the worker dequantises, undoes the wavelet and
  // component transforms and converts on the device (ocr_pipe_stage_batch)
  std::shared_ptr<j2k::Frame> j2k;
  // a JPEG 2000 file after tier-2 only (boxes, markers, packet headers): the worker decodes the code blocks on the device as
  // well, then goes on as for j2k (ocr_pipe_stage_batch, OCR_FRAME_J2K_CODED)
  std::shared_ptr<j2k::Coded> j2k_coded;
  Image() = default;
  explicit Image(const ImageView& v) : rows(v.rows), cols(v.cols) {
    if (!v.empty()) {
      pixels.resize((size_t)rows * cols * 3);
      for (int y = 0; y < rows; ++y) memcpy(&pixels[(size_t)y * cols * 3], v.data + (size_t)y * v.step, (size_t)cols * 3);
    }
  }
  ImageView view() const { return ImageView{pixels.data(), rows, cols, (size_t)cols * 3}; }
  bool empty() const { return pixels.empty() && !jpeg && !png && !raw && !tiff && !webp && !vp8 && !j2k && !j2k_coded && !tiff_coded && !tiff_deflate && !tiff_fax; }
  bool device_decodable() const { return pixels.empty() && (jpeg || png || raw || tiff || webp || vp8 || j2k || j2k_coded || tiff_coded || tiff_deflate || tiff_fax); }
  void materialise() {  // the pixel half of the JPEG / PNG / BMP / PNM / TIFF / WebP on the host
    if (!device_decodable()) return;
    if (j2k_coded) {
      j2k::Frame f;
      if (!j2k::finish_coded(*j2k_coded, f) || !j2k::pixels(f, pixels)) throw std::runtime_error("JPEG 2000 conversion failed");
      j2k_coded.reset();
      return;
    }
    if (j2k) {
      if (!j2k::pixels(*j2k, pixels)) throw std::runtime_error("JPEG 2000 conversion failed");
      j2k.reset();
      return;
    }
    if (vp8) {
      if (!vp8::pixels(*vp8, pixels)) throw std::runtime_error("WebP conversion failed");
      vp8.reset();
      return;
    }
    if (webp) {
      if (!webp::pixels(*webp, pixels)) throw std::runtime_error("WebP conversion failed");
      webp.reset();
      return;
    }
    if (tiff_deflate) {
      tiff::Frame f;
      if (!tiff::inflate_all(*tiff_deflate, f) || !tiff::pixels(f, pixels)) throw std::runtime_error("TIFF conversion failed");
      tiff_deflate.reset();
      return;
    }
    if (tiff_fax) {
      tiff::Frame f;
      if (!tiff::unfax_all(*tiff_fax, f) || !tiff::pixels(f, pixels)) throw std::runtime_error("TIFF conversion failed");
      tiff_fax.reset();
      return;
    }
    if (tiff_coded) {
      tiff::Frame f;
      if (!tiff::expand(*tiff_coded, f) || !tiff::pixels(f, pixels)) throw std::runtime_error("TIFF conversion failed");
      tiff_coded.reset();
      return;
    }
    if (tiff) {
      if (!tiff::pixels(*tiff, pixels)) throw std::runtime_error("TIFF conversion failed");
      tiff.reset();
      return;
    }
    if (raw) {
      if (!raw::pixels(*raw, pixels)) throw std::runtime_error("BMP / PNM conversion failed");
      raw.reset();
      return;
    }
    if (png) {
      if (!png::pixels(*png, pixels)) throw std::runtime_error("PNG reconstruction failed");
      png.reset();
      return;
    }
    if (!jpeg::Decoder::pixels(*jpeg, pixels, rows, cols)) throw std::runtime_error("JPEG reconstruction failed");
    jpeg.reset();
  }
  void materialize() { materialise(); }
  ocr_png_frame png_frame() const {  // only when png
    static_assert(sizeof(png::Segment) == sizeof(ocr_png_segment), "png::Segment is ocr_png_segment");
    ocr_png_frame d;
    memset(&d, 0, sizeof d);
    d.width = png->width; d.height = png->height; d.bit_depth = png->bit_depth; d.color_type = png->color_type; d.interlace = png->interlace;
    memcpy(d.palette, png->palette, sizeof d.palette);
    d.data = png->data.data(); d.data_len = png->data.size();
    d.segments = reinterpret_cast<const ocr_png_segment*>(png->segments.data()); d.nsegments = (int)png->segments.size();
    return d;
  }
  ocr_raw_frame raw_frame() const {  // only when raw
    static_assert((int)raw::kKinds == (int)OCR_RAW_BIT1_INV + 1 && (int)raw::RGB48BE == (int)OCR_RAW_RGB48BE, "raw::Kind is ocr_raw_kind");
    ocr_raw_frame d;
    memset(&d, 0, sizeof d);
    d.width = raw->width; d.height = raw->height; d.kind = raw->kind; d.bottom_up = raw->bottom_up; d.row_stride = raw->row_stride;
    memcpy(d.palette, raw->palette, sizeof d.palette);
    d.data = raw->data.data(); d.data_len = raw->data.size();
    return d;
  }
  ocr_tiff_coded tiff_coded_frame() const { return coded_frame_of(*tiff_coded); }      // only when tiff_coded
  ocr_tiff_coded tiff_deflate_frame() const { return coded_frame_of(*tiff_deflate); }  // only when tiff_deflate
  ocr_tiff_fax tiff_fax_frame() const {  // only when tiff_fax
    ocr_tiff_fax d;
    memset(&d, 0, sizeof d);
    d.coded = coded_frame_of(*tiff_fax);
    d.t4_options = tiff_fax->t4_options;
    return d;
  }
  static ocr_tiff_coded coded_frame_of(const tiff::Coded& c) {
    static_assert(sizeof(tiff::Chunk) == sizeof(ocr_tiff_chunk), "tiff::Chunk is ocr_tiff_chunk");
    const tiff::Frame& f = c.frame;
    ocr_tiff_coded d;
    memset(&d, 0, sizeof d);
    d.frame.width = f.width; d.frame.height = f.height; d.frame.photometric = f.photometric; d.frame.bits_per_sample = f.bits;
    d.frame.samples_per_pixel = f.samples; d.frame.planar = f.planar; d.frame.predictor = f.predictor; d.frame.big_endian = f.big_endian;
    d.frame.premultiply = f.premultiply; d.frame.tile_width = f.tile_width; d.frame.tile_height = f.tile_height;
    memcpy(d.frame.palette, f.palette, sizeof d.frame.palette);
    d.compression = c.compression;
    d.chunks = (const ocr_tiff_chunk*)c.chunks.data(); d.chunks_len = c.chunks.size();
    d.bytes = c.bytes.empty() ? nullptr : c.bytes.data(); d.bytes_len = c.bytes.size();
    return d;
  }
  ocr_tiff_frame tiff_frame() const {  // only when tiff
    ocr_tiff_frame d;
    memset(&d, 0, sizeof d);
    d.width = tiff->width; d.height = tiff->height; d.photometric = tiff->photometric; d.bits_per_sample = tiff->bits;
    d.samples_per_pixel = tiff->samples; d.planar = tiff->planar; d.predictor = tiff->predictor; d.big_endian = tiff->big_endian;
    d.premultiply = tiff->premultiply; d.tile_width = tiff->tile_width; d.tile_height = tiff->tile_height;
    memcpy(d.palette, tiff->palette, sizeof d.palette);
    d.data = tiff->data.data(); d.data_len = tiff->data.size();
    return d;
  }
  ocr_j2k_frame j2k_frame() const {  // only when j2k
    ocr_j2k_frame d;
    memset(&d, 0, sizeof d);
    d.width = j2k->width; d.height = j2k->height; d.x0 = j2k->x0; d.y0 = j2k->y0;
    d.ncomp = j2k->ncomp; d.prec = j2k->prec; d.transform = j2k->transform; d.mct = j2k->mct;
    for (int k = 0; k < 3; ++k) d.chan[k] = j2k->chan[k];
    d.tcs = (const ocr_j2k_tilecomp*)j2k->tcs.data(); d.tcs_len = j2k->tcs.size();
    d.steps = j2k->steps.data(); d.steps_len = j2k->steps.size();
    d.coeffs = j2k->coeffs.data(); d.coeffs_len = j2k->coeffs.size();
    return d;
  }
  ocr_j2k_coded j2k_coded_frame() const {  // only when j2k_coded
    static_assert(sizeof(j2k::CodedBlock) == sizeof(ocr_j2k_cblk), "j2k::CodedBlock is ocr_j2k_cblk");
    const j2k::Frame& f = j2k_coded->frame;
    ocr_j2k_coded d;
    memset(&d, 0, sizeof d);
    d.frame.width = f.width; d.frame.height = f.height; d.frame.x0 = f.x0; d.frame.y0 = f.y0;
    d.frame.ncomp = f.ncomp; d.frame.prec = f.prec; d.frame.transform = f.transform; d.frame.mct = f.mct;
    for (int k = 0; k < 3; ++k) d.frame.chan[k] = f.chan[k];
    d.frame.tcs = (const ocr_j2k_tilecomp*)f.tcs.data(); d.frame.tcs_len = f.tcs.size();
    d.frame.steps = f.steps.data(); d.frame.steps_len = f.steps.size();
    d.frame.coeffs = nullptr; d.frame.coeffs_len = j2k_coded->ncoeffs;
    d.cblks = (const ocr_j2k_cblk*)j2k_coded->cblks.data(); d.cblks_len = j2k_coded->cblks.size();
    d.bytes = j2k_coded->bytes.empty() ? nullptr : j2k_coded->bytes.data(); d.bytes_len = j2k_coded->bytes.size();
    return d;
  }
  ocr_vp8_frame vp8_frame() const {  // only when vp8
    ocr_vp8_frame d;
    memset(&d, 0, sizeof d);
    d.width = vp8->width; d.height = vp8->height; d.filter_type = vp8->filter_type;
    d.mbs = (const ocr_vp8_mb*)vp8->mbs.data(); d.mbs_len = vp8->mbs.size();
    d.coeffs = vp8->coeffs.empty() ? nullptr : vp8->coeffs.data(); d.coeffs_len = vp8->coeffs.size();
    return d;
  }
  ocr_webp_frame webp_frame() const {  // only when webp
    ocr_webp_frame d;
    memset(&d, 0, sizeof d);
    d.width = webp->width; d.height = webp->height;
    d.argb = webp->argb.data(); d.argb_len = webp->argb.size();
    d.ntransforms = (int)webp->transforms.size();
    for (int t = 0; t < d.ntransforms && t < 4; ++t) {
      const webp::Transform& tr = webp->transforms[(size_t)t];
      d.transforms[t].kind = tr.kind; d.transforms[t].bits = tr.bits;
      d.transforms[t].data = tr.data.empty() ? nullptr : tr.data.data(); d.transforms[t].data_len = tr.data.size();
    }
    return d;
  }
  ocr_jpeg_frame jpeg_frame() const {  // only when jpeg: every file the host half reads (any sampling, grey, YCbCr, RGB, CMYK, YCCK)
    ocr_jpeg_frame d;
    memset(&d, 0, sizeof d);
    d.rows = jpeg->rows; d.cols = jpeg->cols; d.ncomp = jpeg->ncomp; d.orientation = jpeg->orientation; d.color = jpeg->color;
    for (int i = 0; i < jpeg->ncomp; ++i) {
      const auto& c = jpeg->comp[i];
      d.comp[i].coef = c.coef.data();
      memcpy(d.comp[i].quant, c.quant, sizeof c.quant);
      d.comp[i].bw = c.bw; d.comp[i].bh = c.bh; d.comp[i].dw = c.dw; d.comp[i].dh = c.dh; d.comp[i].h = c.h; d.comp[i].v = c.v;
    }
    return d;
  }
};

// The descriptors of device-decodable images as ocr_pipe_stage_batch takes them: image i is list[i], tagged with its kind.
// The images must outlive the batch (the descriptors point into them).
struct DeviceFrames {
  std::deque<ocr_jpeg_frame> jf;  // (deques: a descriptor stays where it is when the next one is added)
  std::deque<ocr_png_frame> pf;
  std::deque<ocr_raw_frame> rf;
  std::deque<ocr_tiff_frame> tf;
  std::deque<ocr_webp_frame> wf;
  std::deque<ocr_vp8_frame> vf;
  std::deque<ocr_j2k_frame> kf;
  std::deque<ocr_j2k_coded> kcf;
  std::deque<ocr_tiff_coded> tcf, tdf;
  std::deque<ocr_tiff_fax> tff;
  std::vector<ocr_coded_frame> list;
  template <class D>
  void push(std::deque<D>& q, int kind, const D& d) {
    q.push_back(d);
    list.push_back(ocr_coded_frame{kind, &q.back()});
  }
  void add(const Image& im) {  // only when im.device_decodable(); the first form in this order that the image holds
    if (im.j2k_coded) push(kcf, OCR_FRAME_J2K_CODED, im.j2k_coded_frame());
    else if (im.j2k) push(kf, OCR_FRAME_J2K, im.j2k_frame());
    else if (im.vp8) push(vf, OCR_FRAME_VP8, im.vp8_frame());
    else if (im.webp) push(wf, OCR_FRAME_WEBP, im.webp_frame());
    else if (im.tiff_deflate) push(tdf, OCR_FRAME_TIFF_DEFLATE, im.tiff_deflate_frame());
    else if (im.tiff_fax) push(tff, OCR_FRAME_TIFF_FAX, im.tiff_fax_frame());
    else if (im.tiff_coded) push(tcf, OCR_FRAME_TIFF_CODED, im.tiff_coded_frame());
    else if (im.tiff) push(tf, OCR_FRAME_TIFF, im.tiff_frame());
    else if (im.raw) push(rf, OCR_FRAME_RAW, im.raw_frame());
    else if (im.png) push(pf, OCR_FRAME_PNG, im.png_frame());
    else push(jf, OCR_FRAME_JPEG, im.jpeg_frame());
  }
  int stage(ocr_pipe* pipe, int slot) const { return ocr_pipe_stage_batch(pipe, slot, list.data(), (int)list.size()); }
};

inline void check_ocr(int rc, const char* what) {
  if (rc != OCR_OK) throw std::runtime_error(std::string(what) + ": " + ocr_last_error());
}

// Utility (the hot subset of /root/reference/include/paddle_ocr/utility.h)
class Utility {
 public:
  // Utility::GetRotateCropImage (utility.cpp:137-190): perspective-rectified crop of one det box.
  // Throws where the reference would die inside cv::Mat::operator() (box outside the image / empty).
  static Image GetRotateCropImage(const ImageView& srcimage, const std::vector<std::vector<int>>& box) {
    if (srcimage.empty() || box.size() != 4) throw std::runtime_error("GetRotateCropImage: bad input");
    int32_t b[8];
    for (int i = 0; i < 4; ++i) { b[2 * i] = box[i].at(0); b[2 * i + 1] = box[i].at(1); }
    Image out;
    check_ocr(ocr_rotate_crop_shape(srcimage.rows, srcimage.cols, b, &out.rows, &out.cols), "GetRotateCropImage");
    out.pixels.resize((size_t)out.rows * out.cols * 3);
    size_t off[2];
    int r, c;
    check_ocr(ocr_rotate_crop(srcimage.data, srcimage.rows, srcimage.cols, srcimage.step, b, 1, out.pixels.data(), out.pixels.size(),
                              off, &r, &c), "GetRotateCropImage");
    return out;
  }
};

class DBDetector {
 public:
  // Same parameter list as the reference constructor (ocr_det.h:60-75).  use_gpu must be true: this
  // build is the GPU path; gpu_mem / cpu threads / mkldnn / tensorrt are accepted and ignored.
  explicit DBDetector(const std::string& model_dir, const bool& use_gpu, const int& gpu_id, const int& /*gpu_mem*/,
                      const int& /*cpu_math_library_num_threads*/, const bool& /*use_mkldnn*/, const std::string& limit_type,
                      const int& limit_side_len, const double& det_db_thresh, const double& det_db_box_thresh,
                      const double& det_db_unclip_ratio, const std::string& det_db_score_mode, const bool& use_dilation,
                      const bool& /*use_tensorrt*/, const std::string& precision) {
    if (!use_gpu) throw std::runtime_error("DBDetector: this build has no CPU path (use_gpu must be true)");
    ocr_det_cfg c;
    ocr_det_cfg_default(&c);
    c.model_dir = model_dir.c_str(); c.device_id = gpu_id; c.limit_type = limit_type.c_str();
    c.limit_side_len = limit_side_len; c.det_db_thresh = det_db_thresh; c.det_db_box_thresh = det_db_box_thresh;
    c.det_db_unclip_ratio = det_db_unclip_ratio; c.det_db_score_mode = det_db_score_mode.c_str();
    c.use_dilation = use_dilation; c.precision = precision.c_str();
    check_ocr(ocr_det_create(&c, &h_), "DBDetector");  // the reference exit(1)s here (ocr_det.cpp:41-45); we throw
  }
  ~DBDetector() { ocr_det_destroy(h_); }
  DBDetector(const DBDetector&) = delete;
  DBDetector& operator=(const DBDetector&) = delete;

  // void Run(const cv::Mat&, vector<vector<vector<int>>>& boxes, vector<double>& times)  (ocr_det.h:95-97)
  void Run(const ImageView& img, std::vector<std::vector<std::vector<int>>>& boxes, std::vector<double>& times) {
    std::vector<int32_t> flat(1000 * 8);
    int n = 0;
    double t[3] = {0, 0, 0};
    ocr_img im = img.c();
    check_ocr(ocr_det_run(h_, &im, flat.data(), 1000, &n, t), "DBDetector::Run");
    boxes.clear();
    for (int i = 0; i < n; ++i) {
      std::vector<std::vector<int>> b(4, std::vector<int>(2));
      for (int k = 0; k < 4; ++k) { b[k][0] = flat[i * 8 + 2 * k]; b[k][1] = flat[i * 8 + 2 * k + 1]; }
      boxes.emplace_back(std::move(b));
    }
    times.insert(times.end(), t, t + 3);
  }

 private:
  ocr_det* h_ = nullptr;
};

class Classifier {
 public:
  explicit Classifier(const std::string& model_dir, const bool& use_gpu, const int& gpu_id, const int& /*gpu_mem*/,
                      const int& /*cpu_math_library_num_threads*/, const bool& /*use_mkldnn*/, const double& cls_thresh,
                      const bool& /*use_tensorrt*/, const std::string& precision, const int& cls_batch_num) {
    if (!use_gpu) throw std::runtime_error("Classifier: this build has no CPU path (use_gpu must be true)");
    ocr_cls_cfg c;
    ocr_cls_cfg_default(&c);
    c.model_dir = model_dir.c_str(); c.device_id = gpu_id; c.cls_thresh = cls_thresh; c.cls_batch_num = cls_batch_num;
    c.precision = precision.c_str();
    check_ocr(ocr_cls_create(&c, &h_), "Classifier");
  }
  ~Classifier() { ocr_cls_destroy(h_); }
  Classifier(const Classifier&) = delete;
  Classifier& operator=(const Classifier&) = delete;
  // outputs are pre-sized by the caller (ocr_worker.cpp:271-272)
  void Run(const std::vector<ImageView>& img_list, std::vector<int>& cls_labels, std::vector<float>& cls_scores,
           std::vector<double>& times) {
    std::vector<ocr_img> v;
    for (auto& i : img_list) v.push_back(i.c());
    double t[3] = {0, 0, 0};
    check_ocr(ocr_cls_run(h_, v.data(), (int)v.size(), cls_labels.data(), cls_scores.data(), t), "Classifier::Run");
    times.insert(times.end(), t, t + 3);
  }

 private:
  ocr_cls* h_ = nullptr;
};

class CRNNRecognizer {
 public:
  explicit CRNNRecognizer(const std::string& model_dir, const bool& use_gpu, const int& gpu_id, const int& /*gpu_mem*/,
                          const int& /*cpu_math_library_num_threads*/, const bool& /*use_mkldnn*/,
                          const std::string& label_path, const bool& /*use_tensorrt*/, const std::string& precision,
                          const int& rec_batch_num, const int& rec_img_h, const int& rec_img_w) {
    if (!use_gpu) throw std::runtime_error("CRNNRecognizer: this build has no CPU path (use_gpu must be true)");
    ocr_rec_cfg c;
    ocr_rec_cfg_default(&c);
    c.model_dir = model_dir.c_str(); c.device_id = gpu_id; c.label_path = label_path.c_str();
    c.rec_batch_num = rec_batch_num; c.rec_img_h = rec_img_h; c.rec_img_w = rec_img_w; c.precision = precision.c_str();
    check_ocr(ocr_rec_create(&c, &h_), "CRNNRecognizer");
  }
  ~CRNNRecognizer() { ocr_rec_destroy(h_); }
  CRNNRecognizer(const CRNNRecognizer&) = delete;
  CRNNRecognizer& operator=(const CRNNRecognizer&) = delete;
  // rec_texts / rec_text_scores are pre-sized by the caller (ocr_worker.cpp:286-287); lines whose
  // score would be NaN keep their previous content, like the reference's `continue` (ocr_rec.cpp:123-125)
  void Run(const std::vector<ImageView>& img_list, std::vector<std::string>& rec_texts, std::vector<float>& rec_text_scores,
           std::vector<double>& times) {
    const int n = (int)img_list.size(), max_len = 512;
    std::vector<ocr_img> v;
    for (auto& i : img_list) v.push_back(i.c());
    std::vector<int32_t> ids((size_t)n * max_len);
    std::vector<int> lens(n);
    std::vector<float> scores(n);
    double t[3] = {0, 0, 0};
    check_ocr(ocr_rec_run(h_, v.data(), n, ids.data(), max_len, lens.data(), scores.data(), t), "CRNNRecognizer::Run");
    for (int i = 0; i < n; ++i) {
      if (lens[i] == 0) continue;
      std::string s;
      for (int k = 0; k < lens[i]; ++k) s += ocr_rec_label(h_, ids[(size_t)i * max_len + k]);
      rec_texts[i] = std::move(s);
      rec_text_scores[i] = scores[i];
    }
    times.insert(times.end(), t, t + 3);
  }
  // Per-character evidence of a line (extension; ocr_rec_run_chars): for kept character j its class id, the CTC step it
  // came from, the length of its run of equal arg maxes, the max-probability of that step, and - topk > 0 - the topk
  // best classes of that step with their probabilities (rank 0 = the character itself; ranks > 0 are estimates).
  // geom = {T, tensor_w, resize_w}: the character spans tensor columns [step, step + nsteps) * tensor_w / T.
  struct LineChars {
    std::vector<int> ids, steps, nsteps;
    std::vector<float> probs;
    std::vector<std::vector<int>> alt_ids;
    std::vector<std::vector<float>> alt_probs;
    int geom[3] = {0, 0, 0};
  };
  // Run plus `chars` (resized to img_list.size()); texts and scores are Run's
  void RunChars(const std::vector<ImageView>& img_list, std::vector<std::string>& rec_texts, std::vector<float>& rec_text_scores,
                std::vector<LineChars>& chars, int topk, std::vector<double>& times) {
    const int n = (int)img_list.size(), max_len = 512, kk = topk > 0 ? topk : 1;
    std::vector<ocr_img> v;
    for (auto& i : img_list) v.push_back(i.c());
    std::vector<int32_t> ids((size_t)n * max_len), steps(ids.size()), nsteps(ids.size()), geom((size_t)n * 3), alt_ids(ids.size() * kk);
    std::vector<int> lens(n);
    std::vector<float> scores(n), probs(ids.size()), alt_probs(ids.size() * kk);
    double t[3] = {0, 0, 0};
    check_ocr(ocr_rec_run_chars(h_, v.data(), n, ids.data(), max_len, lens.data(), scores.data(), steps.data(), nsteps.data(), probs.data(),
                                geom.data(), topk, alt_ids.data(), alt_probs.data(), t), "CRNNRecognizer::RunChars");
    chars.assign(n, LineChars());
    for (int i = 0; i < n; ++i) {
      LineChars& c = chars[i];
      for (int k = 0; k < 3; ++k) c.geom[k] = geom[(size_t)i * 3 + k];
      if (lens[i] == 0) continue;
      std::string s;
      for (int k = 0; k < lens[i]; ++k) {
        const size_t q = (size_t)i * max_len + k;
        s += ocr_rec_label(h_, ids[q]);
        c.ids.push_back(ids[q]); c.steps.push_back(steps[q]); c.nsteps.push_back(nsteps[q]); c.probs.push_back(probs[q]);
        if (topk > 0) {
          c.alt_ids.emplace_back(alt_ids.begin() + q * topk, alt_ids.begin() + (q + 1) * topk);
          c.alt_probs.emplace_back(alt_probs.begin() + q * topk, alt_probs.begin() + (q + 1) * topk);
        }
      }
      rec_texts[i] = std::move(s);
      rec_text_scores[i] = scores[i];
    }
    times.insert(times.end(), t, t + 3);
  }

 private:
  ocr_rec* h_ = nullptr;
};

// ---------------------------------------------------------------- worker (ocr_worker.h:22-94)
struct OCRRequest {
  int request_id;
  Image image_data;  // deep copy, like `image_data(img.clone())`
  std::promise<std::string> result_promise;
  OCRRequest(int id, const ImageView& img) : request_id(id), image_data(img) {}
  OCRRequest(int id, Image&& img) : request_id(id), image_data(std::move(img)) {}  // keeps a JPEG coefficient payload
};
struct CharResult {  // extension (OCRWorker::setCharBoxes): one kept character of a word
  std::vector<std::vector<int>> box;  // 4 points in source-image coordinates, reading orientation
  float confidence;                   // the max-probability of the CTC step the character came from
};
struct WordResult {
  std::string text;
  std::vector<std::vector<int>> box;
  float confidence;
  std::vector<CharResult> chars;  // filled only when the worker's char_boxes setting is on
};
struct OCRResult {
  int request_id = 0;
  bool success = false;
  int width = 0, height = 0;
  std::string error_message;
  std::vector<WordResult> words;
  double processing_time_ms = 0;
  bool char_boxes = false;  // the words carry `chars`: the JSON gains a "chars" array per word
};

namespace detail {
inline void json_escape(std::string& o, const std::string& s) {
  o += '"';
  for (unsigned char ch : s) {
    switch (ch) {
      case '"': o += "\\\""; break;
      case '\\': o += "\\\\"; break;
      case '\n': o += "\\n"; break;
      case '\r': o += "\\r"; break;
      case '\t': o += "\\t"; break;
      default:
        if (ch < 0x20) { char b[8]; snprintf(b, sizeof b, "\\u%04x", ch); o += b; }
        else o += (char)ch;  // emitUTF8 = true (ocr_worker.cpp:188)
    }
  }
  o += '"';
}
// keys and order as jsoncpp emits them (alphabetical), no indentation (ocr_worker.cpp:155-190)
inline std::string result_json(const OCRResult& r, int worker_id) {
  std::string o = "{";
  char buf[64];
  if (!r.success) { o += "\"error\":"; json_escape(o, r.error_message); o += ","; }
  snprintf(buf, sizeof buf, "\"height\":%d,", r.height); o += buf;
  snprintf(buf, sizeof buf, "\"processing_time_ms\":%.17g,", r.processing_time_ms); o += buf;
  snprintf(buf, sizeof buf, "\"request_id\":%d,", r.request_id); o += buf;
  o += std::string("\"success\":") + (r.success ? "true" : "false") + ",";
  snprintf(buf, sizeof buf, "\"width\":%d,", r.width); o += buf;
  if (r.success) {
    o += "\"words\":[";
    for (size_t i = 0; i < r.words.size(); ++i) {
      const WordResult& w = r.words[i];
      if (i) o += ",";
      o += "{\"box\":[";
      for (size_t k = 0; k < w.box.size(); ++k) {
        snprintf(buf, sizeof buf, "%s[%d,%d]", k ? "," : "", w.box[k][0], w.box[k][1]);
        o += buf;
      }
      o += "],";
      if (r.char_boxes) {  // (alphabetical: box, chars, confidence, text)
        o += "\"chars\":[";
        for (size_t c = 0; c < w.chars.size(); ++c) {
          o += c ? ",{\"box\":[" : "{\"box\":[";
          for (size_t k = 0; k < w.chars[c].box.size(); ++k) {
            snprintf(buf, sizeof buf, "%s[%d,%d]", k ? "," : "", w.chars[c].box[k][0], w.chars[c].box[k][1]);
            o += buf;
          }
          snprintf(buf, sizeof buf, "],\"confidence\":%.17g}", (double)w.chars[c].confidence);
          o += buf;
        }
        o += "],";
      }
      snprintf(buf, sizeof buf, "\"confidence\":%.17g,\"text\":", (double)w.confidence);
      o += buf;
      json_escape(o, w.text);
      o += "}";
    }
    o += "],";
  }
  snprintf(buf, sizeof buf, "\"worker_id\":%d}", worker_id); o += buf;
  return o;
}
}  // namespace detail

class OCRWorker {
 public:
  // OCRWorker(worker_id, model_dir, use_gpu, gpu_id = 0, enable_cls = false); hyper-parameters are the
  // literals of the reference constructor (ocr_worker.cpp:21-63) — they are ocr_pipe_cfg_default().
  // rotate_crops (extension, default off): crops through Utility::GetRotateCropImage instead of ROI views.
  // max_batch (extension): the worker thread takes up to this many QUEUED requests at once and runs them
  // as one ocr_pipe_run - the GPU is fed whole batches under concurrent load, a lone request is still
  // served immediately (nothing ever waits for a batch to fill).  Per-image results do not depend on what
  // else is in the batch (tests/test_gpu_parity.py, tests/test_ipc_service.py).  0 = OCR_WORKER_MAX_BATCH
  // from the environment, else 16; 1 = the reference's one-request-at-a-time loop.  (16, not 32, since round 4: under
  // 8 .. 96 closed-loop clients the saturated rate is the same, 470-476 requests/s, and the tail is shorter - p99 at 64
  // clients 186 ms against 241 - because a request that just missed a batch waits for a shorter one; profiles/r4_service_sweep.jsonl)
  OCRWorker(int worker_id, const std::string& model_dir, bool use_gpu, int gpu_id = 0, bool enable_cls = false,
            bool rotate_crops = false, int max_batch = 0)
      : worker_id_(worker_id), running_(false), is_idle_(true) {
    if (max_batch <= 0) {
      const char* e = getenv("OCR_WORKER_MAX_BATCH");
      max_batch = e ? atoi(e) : 16;
    }
    max_batch_ = max_batch < 1 ? 1 : (max_batch > 256 ? 256 : max_batch);  // result buffers: 1 MB of ids per image
    gpu_id_ = gpu_id;
    if (!use_gpu) throw std::runtime_error("OCRWorker: this build has no CPU path (use_gpu must be true)");
    det_dir_ = model_dir + "/det"; cls_dir_ = model_dir + "/cls"; rec_dir_ = model_dir + "/rec";
    dict_ = model_dir + "/rec/ppocr_keys_v1.txt";
    ocr_pipe_cfg c;
    ocr_pipe_cfg_default(&c);
    c.det.model_dir = det_dir_.c_str(); c.det.device_id = gpu_id;
    c.cls.model_dir = cls_dir_.c_str();
    c.rec.model_dir = rec_dir_.c_str(); c.rec.label_path = dict_.c_str();
    c.enable_cls = enable_cls;
    c.crop_mode = rotate_crops ? OCR_CROP_ROTATE : OCR_CROP_BOUNDING_RECT;
    // The reference hard-codes the model hyper-parameters in OCRWorker::OCRWorker (src/ocr_worker.cpp:21-63: limit 512,
    // rec 28x192, cls off) and ocr_pipe_cfg_default carries those literals.  Extension for load tests of other
    // operating points (tools/service_load.py): OCR_WORKER_DET_LIMIT, OCR_WORKER_REC_H / _W, OCR_WORKER_CLS=1.
    if (const char* e = getenv("OCR_WORKER_DET_LIMIT")) if (atoi(e) >= 32) c.det.limit_side_len = atoi(e);
    if (const char* e = getenv("OCR_WORKER_REC_H")) if (atoi(e) >= 8) c.rec.rec_img_h = atoi(e);
    if (const char* e = getenv("OCR_WORKER_REC_W")) if (atoi(e) >= 8) c.rec.rec_img_w = atoi(e);
    if (const char* e = getenv("OCR_WORKER_CLS")) if (e[0] == '1') c.enable_cls = 1;
    // (the reference's worker passes the literal "fp32" to its three stage constructors, ocr_worker.cpp:34-60; the stages'
    // own parameter takes "fp16" - OCR_WORKER_PRECISION=fp16 hands it to all three)
    if (const char* e = getenv("OCR_WORKER_PRECISION")) {
      precision_ = e;
      c.det.precision = c.cls.precision = c.rec.precision = precision_.c_str();
    }
    check_ocr(ocr_pipe_create(&c, &pipe_), "OCRWorker");
  }
  virtual ~OCRWorker() { stop(); ocr_pipe_destroy(pipe_); }

  void start() {
    if (running_) return;
    running_ = true;
    worker_thread_ = std::thread(&OCRWorker::workerLoop, this);
  }
  void stop() {
    {
      // under the queue mutex: a worker between its predicate check and its wait would otherwise miss the wake-up
      std::lock_guard<std::mutex> lock(queue_mutex_);
      if (!running_) return;
      running_ = false;
    }
    cv_.notify_all();
    if (worker_thread_.joinable()) worker_thread_.join();
    // requests still queued get an answer, not a broken promise
    std::queue<std::shared_ptr<OCRRequest>> rest;
    { std::lock_guard<std::mutex> lock(queue_mutex_); rest.swap(request_queue_); }
    for (; !rest.empty(); rest.pop()) {
      OCRResult r;
      r.request_id = rest.front()->request_id;
      r.success = false;
      r.error_message = "worker stopped before the request was processed";
      rest.front()->result_promise.set_value(detail::result_json(r, worker_id_));
    }
  }
  void addRequest(std::shared_ptr<OCRRequest> request) {
    { std::lock_guard<std::mutex> lock(queue_mutex_); request_queue_.push(request); }
    cv_.notify_one();
  }
  // char_boxes (extension, default off; set before start()): every word of a reply carries its characters' boxes in
  // source-image coordinates and their confidences (ocr_pipe_run_chars) - "chars":[{"box":[[x,y]x4],"confidence":p},..]
  // in the JSON.  Off, the JSON is byte for byte what it was.  JPEG requests are then decoded on the host.
  void setCharBoxes(bool on) { char_boxes_ = on; }
  bool charBoxes() const { return char_boxes_; }
  bool isIdle() const { return is_idle_; }
  int getWorkerId() const { return worker_id_; }
  int getGpuId() const { return gpu_id_; }
  // load figures for the pool's dispatch and its statistics (round 6): requests waiting in this worker's queue, plus the
  // batch it is running; requests it has answered
  int queueDepth() {
    std::lock_guard<std::mutex> lock(queue_mutex_);
    return (int)request_queue_.size() + in_flight_.load();
  }
  long requestsServed() const { return served_.load(); }

  // processRequest (ocr_worker.cpp:213-311) — public here so tests can call it without the thread
  OCRResult processRequest(const OCRRequest& request) {
    const auto t0 = std::chrono::high_resolution_clock::now();
    OCRResult result;
    result.request_id = request.request_id;
    result.success = false;
    if (request.image_data.empty()) { result.error_message = "Empty image data provided"; return result; }
    result.width = request.image_data.cols;
    result.height = request.image_data.rows;
    std::vector<ocr_word> words(1000);
    std::vector<int32_t> ids(1000 * 256);
    std::vector<ocr_char> chars(char_boxes_ ? ids.size() : 0);
    int off = 0, n = 0;
    int rc;
    if (char_boxes_) {
      if (!materialised(request, result)) return result;
      ocr_img im = request.image_data.view().c();
      rc = ocr_pipe_run_chars(pipe_, &im, 1, words.data(), (int)words.size(), &off, &n, ids.data(), (int)ids.size(), chars.data(), nullptr);
    } else
    if (request.image_data.device_decodable()) {  // JPEG, PNG, BMP / PNM: pixels are produced on the device, straight into the staging slot
      DeviceFrames frames;
      frames.add(request.image_data);
      rc = frames.stage(pipe_, 0);
      if (rc == OCR_OK) rc = ocr_pipe_run_staged(pipe_, 0, words.data(), (int)words.size(), &off, &n, ids.data(), (int)ids.size(), nullptr);
      else if (rc == OCR_ERR_ARG && request.image_data.tiff_deflate) {
        // the device refused a stream of a Deflate TIFF: the host is right where the two differ, so zlib decides - a file it
        // refuses too fails here, one it accepts goes on from its pixels
        if (!materialised(request, result)) return result;
        ocr_img im = request.image_data.view().c();
        rc = ocr_pipe_run(pipe_, &im, 1, words.data(), (int)words.size(), &off, &n, ids.data(), (int)ids.size(), nullptr);
      }
    } else {
      ocr_img im = request.image_data.view().c();
      rc = ocr_pipe_run(pipe_, &im, 1, words.data(), (int)words.size(), &off, &n, ids.data(), (int)ids.size(), nullptr);
    }
    if (rc != OCR_OK) { result.error_message = ocr_last_error(); return result; }  // the reference's catch (...) path
    result.success = true;
    result.char_boxes = char_boxes_;
    for (int i = 0; i < n; ++i) {
      WordResult w;
      for (int k = 0; k < words[i].ids_len; ++k) w.text += ocr_pipe_label(pipe_, ids[words[i].ids_off + k]);
      w.confidence = words[i].confidence;
      w.box.assign(4, std::vector<int>(2));
      for (int k = 0; k < 4; ++k) { w.box[k][0] = words[i].box[2 * k]; w.box[k][1] = words[i].box[2 * k + 1]; }
      if (char_boxes_) fill_chars(w, words[i], chars.data());
      result.words.push_back(std::move(w));
    }
    result.processing_time_ms =
        std::chrono::duration<double, std::milli>(std::chrono::high_resolution_clock::now() - t0).count();
    return result;
  }

  // Image::materialise() for a request; false, with the result's error set, where the host refuses the image (a Deflate TIFF
  // with a faulty stream, which nobody has looked at before): that request fails, nothing else does
  static bool materialised(const OCRRequest& request, OCRResult& result) {
    try {
      const_cast<OCRRequest&>(request).image_data.materialise();
      return true;
    } catch (const std::exception& e) {
      result.error_message = e.what();
      return false;
    }
  }

  // The same for several requests in one pipeline run; results[i] belongs to requests[i].  A failure of
  // the batched run (one oversized image, say) falls back to request-by-request processing, so a request
  // fails or succeeds exactly as it would alone.  processing_time_ms is the wall time of the run a request
  // was part of.
  std::vector<OCRResult> processBatch(const std::vector<const OCRRequest*>& requests) {
    const auto t0 = std::chrono::high_resolution_clock::now();
    std::vector<OCRResult> results(requests.size());
    std::vector<ocr_img> imgs;
    DeviceFrames frames;
    std::vector<size_t> owner;
    // a batch of JPEGs, PNGs, raw BMP / PNM frames, TIFF and WebP frames only (of the last three there are none unless OCR_DEVICE_RAW=1 /
    // OCR_DEVICE_TIFF=1 / OCR_DEVICE_WEBP=1: the IPC layer finishes those files on the host) is decoded on the device, in one ocr_pipe_stage_batch call whatever the mix; a batch
    // with other host pixels in it takes the host path for all its images
    bool on_device = !char_boxes_;
    for (size_t i = 0; i < requests.size(); ++i)
      if (!requests[i]->image_data.empty() && !requests[i]->image_data.device_decodable()) on_device = false;
    for (size_t i = 0; i < requests.size(); ++i) {
      results[i].request_id = requests[i]->request_id;
      if (requests[i]->image_data.empty()) { results[i].error_message = "Empty image data provided"; continue; }
      results[i].width = requests[i]->image_data.cols;
      results[i].height = requests[i]->image_data.rows;
      if (on_device) frames.add(requests[i]->image_data);
      else {
        if (!materialised(*requests[i], results[i])) continue;  // (this request fails; the batch goes on without it)
        imgs.push_back(requests[i]->image_data.view().c());
      }
      owner.push_back(i);
    }
    if (owner.empty()) return results;
    if (owner.size() == 1) { results[owner[0]] = processRequest(*requests[owner[0]]); return results; }
    const int k = (int)owner.size();
    // result buffers live with the worker (grown once): 1000 words of up to 256 ids per image, as processRequest
    if (batch_words_.size() < (size_t)k * 1000) { batch_words_.resize((size_t)k * 1000); batch_ids_.resize((size_t)k * 1000 * 256); }
    std::vector<ocr_word>& words = batch_words_;
    std::vector<int32_t>& ids = batch_ids_;
    std::vector<int> off(k), cnt(k);
    if (char_boxes_ && batch_chars_.size() < ids.size()) batch_chars_.resize(ids.size());
    int rc;
    if (char_boxes_) {
      rc = ocr_pipe_run_chars(pipe_, imgs.data(), k, words.data(), k * 1000, off.data(), cnt.data(), ids.data(), k * 1000 * 256, batch_chars_.data(), nullptr);
    } else
    if (on_device) {
      rc = frames.stage(pipe_, 0);
      if (rc == OCR_OK) rc = ocr_pipe_run_staged(pipe_, 0, words.data(), k * 1000, off.data(), cnt.data(), ids.data(), k * 1000 * 256, nullptr);
    } else {
      rc = ocr_pipe_run(pipe_, imgs.data(), k, words.data(), k * 1000, off.data(), cnt.data(), ids.data(), k * 1000 * 256, nullptr);
    }
    if (rc != OCR_OK) {
      for (size_t j = 0; j < owner.size(); ++j) results[owner[j]] = processRequest(*requests[owner[j]]);
      return results;
    }
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::high_resolution_clock::now() - t0).count();
    for (int j = 0; j < k; ++j) {
      OCRResult& r = results[owner[j]];
      r.success = true;
      r.char_boxes = char_boxes_;
      for (int i = off[j]; i < off[j] + cnt[j]; ++i) {
        WordResult w;
        for (int q = 0; q < words[i].ids_len; ++q) w.text += ocr_pipe_label(pipe_, ids[words[i].ids_off + q]);
        w.confidence = words[i].confidence;
        w.box.assign(4, std::vector<int>(2));
        for (int q = 0; q < 4; ++q) { w.box[q][0] = words[i].box[2 * q]; w.box[q][1] = words[i].box[2 * q + 1]; }
        if (char_boxes_) fill_chars(w, words[i], batch_chars_.data());
        r.words.push_back(std::move(w));
      }
      r.processing_time_ms = ms;
    }
    return results;
  }
  int maxBatch() const { return max_batch_; }

  // the characters of one word out of the pipeline's ocr_char array (parallel to the class ids)
  static void fill_chars(WordResult& w, const ocr_word& word, const ocr_char* chars) {
    for (int k = 0; k < word.ids_len; ++k) {
      const ocr_char& c = chars[word.ids_off + k];
      CharResult cr;
      cr.confidence = c.prob;
      cr.box.assign(4, std::vector<int>(2));
      for (int q = 0; q < 4; ++q) { cr.box[q][0] = c.quad[2 * q]; cr.box[q][1] = c.quad[2 * q + 1]; }
      w.chars.push_back(std::move(cr));
    }
  }

 private:
  void workerLoop() {
    while (running_) {
      std::vector<std::shared_ptr<OCRRequest>> batch;
      {
        std::unique_lock<std::mutex> lock(queue_mutex_);
        cv_.wait(lock, [this] { return !request_queue_.empty() || !running_; });
        if (!running_) break;
        auto take = [&] {
          while (!request_queue_.empty() && (int)batch.size() < max_batch_) {
            batch.push_back(request_queue_.front());
            request_queue_.pop();
          }
        };
        take();
        if (!batch.empty()) { is_idle_ = false; in_flight_ = (int)batch.size(); }
      }
      if (batch.empty()) continue;
      std::vector<const OCRRequest*> ptrs;
      for (auto& b : batch) ptrs.push_back(b.get());
      std::vector<OCRResult> rs;
      try {
        rs = processBatch(ptrs);
      } catch (const std::exception& e) {
        rs.assign(batch.size(), OCRResult());
        for (size_t i = 0; i < batch.size(); ++i) {
          rs[i].request_id = batch[i]->request_id;
          rs[i].success = false;
          rs[i].error_message = e.what();
        }
      }
      for (size_t i = 0; i < batch.size(); ++i) batch[i]->result_promise.set_value(detail::result_json(rs[i], worker_id_));
      served_ += (long)batch.size();
      in_flight_ = 0;
      is_idle_ = true;
    }
  }

  int worker_id_;
  int gpu_id_ = 0;
  int max_batch_ = 1;
  std::string precision_;  // OCR_WORKER_PRECISION (kept alive for the configuration's pointers)
  std::vector<ocr_word> batch_words_;
  std::vector<int32_t> batch_ids_;
  std::vector<ocr_char> batch_chars_;
  bool char_boxes_ = false;
  std::atomic<bool> running_, is_idle_;
  std::atomic<int> in_flight_{0};
  std::atomic<long> served_{0};
  std::thread worker_thread_;
  std::queue<std::shared_ptr<OCRRequest>> request_queue_;
  std::mutex queue_mutex_;
  std::condition_variable cv_;
  ocr_pipe* pipe_ = nullptr;
  std::string det_dir_, cls_dir_, rec_dir_, dict_;
};

// ---------------------------------------------------------------- pool (gpu_worker_pool.h:14-31)
// The reference pins every worker to GPU 0 (gpu_worker_pool.cpp:12-16); here worker i runs on GPU
// i mod ocr_rt_device_count(): whole images are sharded over the node's GPUs, nothing else changes.
class GPUWorkerPool {
 public:
  // Dispatch: the reference's rule (first idle worker, else round robin: gpu_worker_pool.cpp:46-59) is the default.
  // LeastQueued (round 6, an option): the worker with the fewest requests queued or running - under a stream of mixed-size
  // requests round robin hands a slow worker as many requests as a fast one (profiles/r6_pool_load.json has the histograms).
  // OCR_POOL_DISPATCH=least in the environment selects it for pools that do not call setDispatch.
  enum Dispatch { IdleFirstRoundRobin = 0, LeastQueued = 1 };
  GPUWorkerPool(const std::string& model_dir, int num_workers = 2) : next_worker_index_(0) {
    const int ngpu = ocr_rt_device_count();
    if (ngpu <= 0) throw std::runtime_error("GPUWorkerPool: no HIP device visible");
    for (int i = 0; i < num_workers; ++i) workers_.emplace_back(std::make_unique<OCRWorker>(i, model_dir, true, i % ngpu));
    if (const char* e = getenv("OCR_POOL_DISPATCH")) if (e[0] == 'l') dispatch_ = LeastQueued;
    depth_hist_.assign(65, 0);
  }
  ~GPUWorkerPool() { stop(); }
  void start() { for (auto& w : workers_) w->start(); }
  void stop() { for (auto& w : workers_) w->stop(); }
  void setDispatch(Dispatch d) { dispatch_ = d; }
  std::future<std::string> submitRequest(std::shared_ptr<OCRRequest> request) {
    auto future = request->result_promise.get_future();
    getAvailableWorker()->addRequest(request);
    return future;
  }
  int getOptimalWorkerCount() { return ocr_rt_device_count(); }  // declared, never defined in the reference
  int workerDevice(int i) const { return workers_[i]->getGpuId(); }
  int workerCount() const { return (int)workers_.size(); }
  // statistics: requests answered per worker; histogram of the chosen worker's depth (queued + running) at submit time,
  // bucket 64 = 64 or more
  std::vector<long> requestsPerWorker() const { std::vector<long> v; for (auto& w : workers_) v.push_back(w->requestsServed()); return v; }
  std::vector<long> submitDepthHistogram() { std::lock_guard<std::mutex> lock(workers_mutex_); return depth_hist_; }

 private:
  OCRWorker* getAvailableWorker() {
    std::lock_guard<std::mutex> lock(workers_mutex_);
    OCRWorker* pick = nullptr;
    if (dispatch_ == LeastQueued) {
      int best = 1 << 30;
      const int n = (int)workers_.size(), start = next_worker_index_.fetch_add(1) % n;  // (ties: rotate, so that an idle pool still spreads)
      for (int k = 0; k < n; ++k) {
        OCRWorker* w = workers_[(start + k) % n].get();
        const int d = w->queueDepth();
        if (d < best) { best = d; pick = w; }
      }
    } else {  // first idle, else round robin (gpu_worker_pool.cpp:46-59)
      for (auto& w : workers_) if (w->isIdle()) { pick = w.get(); break; }
      if (!pick) pick = workers_[next_worker_index_.fetch_add(1) % (int)workers_.size()].get();
    }
    const int d = pick->queueDepth();
    depth_hist_[d > 64 ? 64 : d]++;
    return pick;
  }
  std::vector<std::unique_ptr<OCRWorker>> workers_;
  std::mutex workers_mutex_;
  std::atomic<int> next_worker_index_;
  Dispatch dispatch_ = IdleFirstRoundRobin;
  std::vector<long> depth_hist_;
};

}  // namespace PaddleOCR
