// Stage objects behind the C-ABI: detector, classifier, recognizer.  Each owns one HIP stream, its
// network and its device buffers ("one handle per host thread").
#pragma once
#include <hip/hip_runtime.h>

#include <memory>
#include <string>
#include <vector>

#include "../../include/ocr_hip.h"
#include "kernels_post.h"
#include "kernels_pre.h"
#include "net.h"
#include "srv_net.h"

namespace ocr {

// growable device buffer
template <class T>
struct DevBuf {
  T* p = nullptr;
  size_t cap = 0;
  ~DevBuf() { if (p) (void)g_free(p); }
  bool ensure(size_t n, std::string& err) {
    if (n <= cap) return true;
    if (p) (void)g_free(p);
    p = nullptr;
    cap = 0;
    hipError_t e = g_malloc(&p, n * sizeof(T));
    if (e != hipSuccess) { err = std::string("hipMalloc: ") + hipGetErrorString(e); return false; }
    cap = n;
    return true;
  }
};

struct StageTimer {  // pre / infer / post in ms from HIP events on the stage's stream
  hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
  bool init(std::string& err);
  ~StageTimer();
  void mark(int i, hipStream_t s) { (void)hipEventRecord(ev[i], s); }
  void read(double times[3]);
};

struct DetConfig {
  std::string model_dir, limit_type = "max", score_mode = "fast", precision = "fp32";
  int device = 0, limit_side_len = 512, use_dilation = 0, max_batch = 1;
  double thresh = 0.2, box_thresh = 0.4, unclip_ratio = 1.8;
  int cv_compat = 410;  // OCR_CV_45 | OCR_CV_410 (resolved: never 0 here)
};

class DetStage {
 public:
  ~DetStage();
  bool create(const DetConfig& cfg, std::string& err, int& code);
  // imgs: `count` same-size host images.  boxes [count][cap][8], n [count].
  int run(const ocr_img* imgs, int count, int32_t* boxes, int cap, int* n, double times[3], std::string& err);
  // the same on images that already sit in device memory (packed BGR rows, one image every img_bytes)
  // prob_override (device, [count][rh][rw] f32, may be null): the benchmark protocol of SURVEY.md §8d —
  // the network still runs, but thresholding / scoring read this map instead of the network's.
  int run_device(const uint8_t* dev_imgs, size_t img_bytes, size_t stride, int rows, int cols, int count, int32_t* boxes,
                 int cap, int* n, double times[3], std::string& err, const float* prob_override = nullptr);
  // ---- batches of MIXED sizes: one ragged network launch for all size groups, post-processing per group -----------
  // A size group = `count` images of rows x cols, packed BGR, starting `off` bytes into the batch's device buffer;
  // prob_off = floats into the benchmark protocol's probability-map buffer (prob_override of run_device).
  struct MixedGroup { int rows, cols, count; size_t off, prob_off; };
  // Enqueues resize + normalise of every group and ONE network pass over all images (Net::run_ragged_images: every
  // image keeps its own size) on this stage's stream and records `done()`; the maps of group i are then at
  // mixed_prob(i) / mixed_bitmap(i).  The caller runs post_group per group - on this stage or, concurrently, on other
  // DetStage instances (their streams wait for done()).
  int mixed_net(const uint8_t* base, const MixedGroup* groups, int ngroups, const float* prob_override, std::string& err);
  const float* mixed_prob(int gi) const { return mixed_probs_[gi]; }
  const uint8_t* mixed_bitmap(int gi) const { return bitmap_.p + mixed_pix_[gi]; }
  hipEvent_t done() const { return mixed_done_; }
  void collect_timings() { net_.collect_timings(); }  // after the stream that ran mixed_net has been synchronised
  // BoxesFromBitmap + FilterTagDetRes of EVERY group of the last mixed_net in one pass (the post-processing kernels
  // take each image's own map size: kernels_post.h, PostImg); boxes [images][cap][8] and n [images] in group order.
  // Not with use_dilation (the 2x2 dilate is per size): the caller then goes through post_group.
  int post_mixed(const MixedGroup* groups, int ngroups, int32_t* boxes, int cap, int* n, std::string& err);
  // BoxesFromBitmap + FilterTagDetRes of one size group whose maps sit in device memory (another stage's mixed_net)
  int post_group(const float* prob, const uint8_t* bitmap, const MixedGroup& g, hipEvent_t wait_for, int32_t* boxes, int cap, int* n,
                 std::string& err);
  // mutable view of the uploaded copies (the request's clone: cls rotation happens in place on it)
  uint8_t* dev_images_mut() { return src_.p; }
  int post_only(const float* prob, int rows, int cols, int src_rows, int src_cols, int32_t* boxes, int cap, int* n,
                std::string& err);
  // Stage tap (ocr_det_post_stages, tests): what the launch sequence of the last post_only left in this stage's buffers for
  // image 0 - nothing is launched.  The first call on a stage arms it (the per-candidate record of kernels_post.h is
  // allocated and handed to the kernels from then on) and is refused like every call that has no recorded post_only before it.
  int post_stages(ocr_post_stages* out, std::string& err);
  // device-resident copy of the last uploaded images (for the fused pipeline)
  const uint8_t* dev_images() const { return src_.p; }
  size_t dev_image_bytes() const { return (size_t)src_rows_ * src_cols_ * 3; }
  hipStream_t stream() const { return stream_; }
  Net& net() { return net_; }
  int last_count = 0, last_h = 0, last_w = 0;
  const float* prob_dev() const { return srv_ ? (const float*)srv_->tensor_ptr(srv_->output_tid()) : net_.tensor_ptr(net_.output_tid()); }
  // the server detector (BASELINE configs[4]: a model directory whose arch.txt says srv_det), or null
  SrvNet* srv() { return srv_.get(); }
  const uint8_t* bitmap_dev() const { return cfg_.use_dilation ? bitmap2_.p : bitmap_.p; }
  const uint8_t* resized_dev() const { return resized_.p; }
  const DetConfig& cfg() const { return cfg_; }
  static void resize_shape(int h, int w, const std::string& limit_type, int limit_side_len, int& rh, int& rw,
                           float& ratio_h, float& ratio_w);

 private:
  bool ensure_post(int count, size_t px, int H, int W, int cap, std::string& err);
  int post_launch(PostArgs a, int count, int32_t* boxes, int cap, int* n, std::string& err);
  int run_post(int count, int H, int W, const float* prob, float ratio_h, float ratio_w, int src_h, int src_w,
               int32_t* boxes, int cap, int* n, std::string& err, const uint8_t* bitmap = nullptr);
  std::vector<size_t> mixed_pix_;            // first pixel of every group in the ragged maps
  const float* mixed_prob_base_ = nullptr;   // what post_mixed's per-image offsets are relative to
  DevBuf<PostImg> post_img_;
  std::vector<const float*> mixed_probs_;
  hipEvent_t mixed_done_ = nullptr;
  DetConfig cfg_;
  Net net_;
  std::unique_ptr<SrvNet> srv_;
  hipStream_t stream_ = nullptr;
  StageTimer timer_;
  DevBuf<float> lut_, x_, prob_in_;
  DevBuf<uint8_t> src_, resized_, bitmap_, bitmap2_, touch_;
  DevBuf<int> labels_, chunk_cnt_, ncont_all_, ncont_, starts_, npts_, poff_, iscratch_, cand_boxes_, cand_valid_, status_, out_boxes_,
      out_n_;
  DevBuf<unsigned long long> pool_;
  DevBuf<unsigned> mask_pool_, mask_top_;
  DevBuf<float> stage_rec_;  // [images][max_cand][POST_REC_FLOATS], only on a stage whose tap has been asked for
  bool tap_armed_ = false, tap_valid_ = false;  // valid: the last post-processing pass was a post_only that recorded
  int tap_h_ = 0, tap_w_ = 0;
  DevBuf<int> pool_need_;   // [images] keys the traced borders of an image would have needed (kernels_post.h)
  size_t mask_words_ = 0;   // words of polygon-score scratch per image in this call
  // words of polygon-score scratch per image: masks + crossing lists of all its borders (8 map areas of bits + slack)
  static size_t mask_words(int H, int W) { return (((size_t)H * W / 4 + (1u << 16)) + 31) & ~(size_t)31; }
  int src_rows_ = 0, src_cols_ = 0;
  int ithresh_ = 0;
  int pool_cap_ = 0;
  int bm_n_ = 0;  // 1 once the fused-bitmap pointer has been handed to the network
};

struct LineSrc {  // a text-line image living in device memory
  const uint8_t* img;
  size_t stride;
  int x, y, w, h;
};

struct RecConfig {
  std::string model_dir, label_path, precision = "fp32";
  int device = 0, batch_num = 16, img_h = 28, img_w = 192;
  int sort_mode = 0;  // OCR_SORT_STD | OCR_SORT_STABLE
};

class RecStage {
 public:
  ~RecStage();
  // Per-character evidence (ocr_rec_run_chars): arrays parallel to ids (n x max_len) - the CTC step a kept character came
  // from, the length of its run of equal arg maxes, pmax of that step; geom per line {T, tensor_w, resize_w}; with
  // topk in 1..8 the topk best classes of that step's logits row (n x max_len x topk).  steps/nsteps/probs/geom may be null.
  struct CharOut {
    int32_t* steps = nullptr;
    int32_t* nsteps = nullptr;
    float* probs = nullptr;
    int32_t* geom = nullptr;
    int topk = 0;
    int32_t* alt_ids = nullptr;
    float* alt_probs = nullptr;
  };
  bool create(const RecConfig& cfg, std::string& err, int& code);
  int run(const ocr_img* imgs, int n, int32_t* ids, int max_len, int* lens, float* scores, double times[3],
          std::string& err);
  // lines already on the device (the stream must be ordered after whatever produced them).
  // seg: offsets of per-image segments (size nimages+1); the reference's aspect-sort / batch-of-16
  // rule is applied inside each segment, launches are shared across segments of equal tensor width.
  int run_lines(const std::vector<LineSrc>& lines, const std::vector<int>& seg, int32_t* ids, int max_len, int* lens,
                float* scores, std::string& err, const CharOut* co = nullptr);
  int run_chars(const ocr_img* imgs, int n, int32_t* ids, int max_len, int* lens, float* scores, const CharOut& co, double times[3],
                std::string& err);
  int run_lines_chars(const std::vector<LineSrc>& lines, const std::vector<int>& seg, int32_t* ids, int max_len, int* lens,
                      float* scores, const CharOut& co, std::string& err) {
    return run_lines(lines, seg, ids, max_len, lens, scores, err, &co);
  }
  // tap: the logits row behind step `step` of line `index` of the last run_chars(topk > 0) with want_taps (C floats)
  int logits_row(int index, int step, float* out, size_t cap_floats, std::string& err);
  bool want_taps = true;
  // Lines per network launch; a longer call is cut into several (rec_plan::plan_slots; ocr_rec_set_launch_lines for tests).
  // Mobile recognizer: bounds the activation arena of one launch - this many 48x320 lines' pixels (~1.2 MB each).
  // Server recognizer (create() sets kSrvLinesPerLaunch): every tensor of a launch is read through one buffer descriptor, which
  // spans less than 0xfffffff0 bytes (srv_kernels.hip, launch_gemm / launch_mlp: "tensor beyond the 4 GB ...").  The largest
  // tensor of srv_rec.plan per 48 x 320 line is an MLP's hidden one in the first stage, [12][80][768] = 737 280 elements
  // (tensors 8, 15, 22; next: qkv [12][80][576], the f32 logits [80][6632]) - 2 949 120 bytes in the f32 twin, 1 474 560 in the
  // f16 build with every tensor materialised (keep_all, OCR_SRV_MLP=0; with the fused MLP it never exists and qkv's
  // 1 105 920 bytes lead).  0xfffffff0 / 2 949 120 = 1456.3 lines: 1024 keeps every build and mode below the guard (3.02 GB),
  // where 4096 lines passed it even in the f16 build (4096 x 1 105 920 = 4.5 GB).  This is arithmetic on the plan: no launch of more
  // than a few lines has run in a test.  A call of more than 1024 lines binds a second batch size (the remainder), which is timed
  // for its tiles like every new one (srv_net.hip, tune).
  static constexpr int kSrvLinesPerLaunch = 1024;
  static_assert((unsigned long long)kSrvLinesPerLaunch * (12 * 80 * 768) * sizeof(float) < 0xfffffff0ull, "a server launch passes the buffer-descriptor guard");
  int max_lines_per_launch = 4096;
  const std::vector<std::string>& labels() const { return labels_; }
  hipStream_t stream() const { return stream_; }
  Net& net() { return net_; }
  SrvNet* srv() { return srv_.get(); }  // the server recognizer (arch.txt: srv_rec), or null
  // per-step taps of the last run, in input order: T per line, amax/pmax concatenated
  std::vector<int> tap_T, tap_off;
  std::vector<int> tap_amax;
  std::vector<float> tap_pmax;

 private:
  struct LinesCtx;  // stages.hip: what the phases of run_lines share
  RecConfig cfg_;
  // One network instance, one stream: the lines of a call run as ONE ragged launch list whatever their tensor widths
  // (run_lines); rounds 1-2 launched once per distinct width on up to six streams ("lanes").
  Net net_;
  std::unique_ptr<SrvNet> srv_;
  hipStream_t stream_ = nullptr;
  StageTimer timer_;
  std::vector<std::string> labels_;
  DevBuf<float> lut_, pmax_, scores_, x_;
  DevBuf<int> amax_, ids_, lens_;
  DevBuf<uint8_t> staging_;
  DevBuf<LineDesc> descs_;
  // run_chars: per kept character step / run length / probability, the top-k classes, and (want_taps) a copy of the
  // logits rows of the last topk run, C floats each, line li's at row tap_row0_[li]
  DevBuf<int> csteps_, cnsteps_, alt_ids_;
  DevBuf<float> cprobs_, alt_probs_, logit_tap_;
  std::vector<long> tap_row0_;
  int tap_C_ = 0;
  bool srv_ctc_ = false;  // the server head's CTC-partials mode outside top-k calls (create)
};

struct ClsConfig {
  std::string model_dir, precision = "fp32";
  int device = 0, batch_num = 8;
  double thresh = 0.98;
};

class ClsStage {
 public:
  ~ClsStage();
  bool create(const ClsConfig& cfg, std::string& err, int& code);
  int run(const ocr_img* imgs, int n, int* labels, float* scores, double times[3], std::string& err);
  int run_lines(const std::vector<LineSrc>& lines, int* labels, float* scores, std::string& err);
  hipStream_t stream() const { return stream_; }
  Net& net() { return net_; }
  std::vector<float> tap_probs;  // [n][2] of the last run

 private:
  ClsConfig cfg_;
  Net net_;
  hipStream_t stream_ = nullptr;
  StageTimer timer_;
  DevBuf<float> lut_, x_, pmax_, probs_;
  DevBuf<int> amax_;
  DevBuf<uint8_t> staging_;
  DevBuf<LineDesc> descs_;
};

// Uploads ROI views into one packed staging buffer and describes them as device lines.
bool upload_lines(const ocr_img* imgs, int n, DevBuf<uint8_t>& staging, std::vector<LineSrc>& out, hipStream_t s,
                  std::string& err);

// 3x256 normalisation LUT: Normalize::Run per byte value (convertTo 1/255, then scale/shift)
std::vector<float> make_norm_lut(const float mean[3], const float scale[3]);
// the table of one stage (its mean / scale literals live here alone): the stages upload it at create, the
// ocr_selftest_*_pre taps launch the pre-processing kernels with it
enum class NormStage { Det, Rec, Cls };
std::vector<float> stage_norm_lut(NormStage st);

}  // namespace ocr
