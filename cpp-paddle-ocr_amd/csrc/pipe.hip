// Fused det -> crop -> [cls -> rotate] -> rec pipeline over device-resident images
// (OCRWorker::processRequest, /root/reference/src/ocr_worker.cpp:213-311) and its C-ABI.
#include <algorithm>
#include <array>
#include <chrono>
#include <cstring>
#include <functional>
#include <map>
#include <memory>
#include <thread>

#include "capi_common.h"
#include "crop.h"
#include "frame_kinds.h"
#include "pipe_plan.h"
#include "rot_groups.h"
#include "stages.h"

using namespace ocr;
using pipe_plan::CharLists;
using WordLists = std::vector<std::vector<ocr_word>>;  // per image, as IdLists: what a run hands to pipe_plan::emit
using IdLists = std::vector<std::vector<int32_t>>;

namespace {
double now_ms() {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// fn(i, message) for i = 0 .. n-1 side by side: 0 on the calling thread, every other on a thread of its own that lives for
// this call; the code and the message of the first i that failed
template <class F>
int run_side_by_side(int n, std::string& err, F fn) {
  std::vector<int> rcs(n, OCR_OK);
  std::vector<std::string> errs(n);
  std::vector<std::thread> th;
  for (int i = 1; i < n; ++i) th.emplace_back([&, i] { rcs[i] = fn(i, errs[i]); });
  rcs[0] = fn(0, errs[0]);
  for (auto& t : th) t.join();
  for (int i = 0; i < n; ++i)
    if (rcs[i]) { err = errs[i]; return rcs[i]; }
  return OCR_OK;
}
}  // namespace

// One staged batch: host images copied into pinned memory and sent to the device on the copy stream, laid out size group by
// size group (pipe_plan::layout).  Two slots = double buffering: batch k+1 is staged (by another host thread) while batch k
// runs - SURVEY.md section 8e's "double-buffered pinned staging".
struct StageSlot {
  using Img = pipe_plan::Img;
  using Group = pipe_plan::Group;
  PinnedStage pinned;  // free again once `ready` has passed (layout() waits for it: pinned.copied is never recorded)
  DevBuf<uint8_t> dev;
  DevBuf<float> probs;
  std::vector<Img> imgs;      // layout order
  std::vector<Group> groups;
  size_t bytes = 0, prob_floats = 0;
  bool has_probs = false, staged = false;
  hipEvent_t ready = nullptr;
  ~StageSlot() { if (ready) (void)hipEventDestroy(ready); }
};

// In-place 180-degree rotations of ROIs in request order (the cls stage: cv::rotate on views that alias their image,
// /root/reference/src/ocr_worker.cpp:255-262).  Only ROIs that intersect constrain each other: the ROIs of a view
// (img pointer + stride identify the image; different views are different images or separate crop buffers and do not
// alias) are grouped into the connected components of "intersects"; a component keeps request order inside one
// workgroup, components run concurrently, ONE launch for the batch.
static int rotate180_in_order(const std::vector<RotDesc>& rd, DevBuf<RotDesc>& scratch, DevBuf<int>& seg_scratch, hipStream_t stream,
                              std::string& err) {
  if (rd.empty()) return OCR_OK;
  const int n = (int)rd.size();
  std::vector<rot_groups::Rect> rects(n);
  std::vector<std::pair<const uint8_t*, size_t>> view(n);
  for (int k = 0; k < n; ++k) {
    rects[k] = rot_groups::Rect{rd[k].x, rd[k].y, rd[k].w, rd[k].h};
    view[k] = {rd[k].img, rd[k].stride};
  }
  // components in order of their first ROI, members in request order
  std::vector<int> order, seg;
  rot_groups::group(rects, view, order, seg);
  std::vector<RotDesc> sorted;
  sorted.reserve(n);
  for (int k : order) sorted.push_back(rd[k]);
  if (!scratch.ensure(sorted.size(), err) || !seg_scratch.ensure(seg.size(), err)) return OCR_ERR_DEVICE;
  if (hipMemcpyAsync(scratch.p, sorted.data(), sorted.size() * sizeof(RotDesc), hipMemcpyHostToDevice, stream) != hipSuccess ||
      hipMemcpyAsync(seg_scratch.p, seg.data(), seg.size() * sizeof(int), hipMemcpyHostToDevice, stream) != hipSuccess) {
    err = "rotation list upload failed";
    return OCR_ERR_DEVICE;
  }
  launch_rotate180_groups(scratch.p, seg_scratch.p, (int)seg.size() - 1, stream);
  if (hipGetLastError() != hipSuccess) { err = "rotation launch failed"; return OCR_ERR_DEVICE; }
  return OCR_OK;
}

// One chain det -> crops -> [cls -> rotate] -> rec (OCRWorker::processRequest) with its own stage objects, streams and
// buffers.  A pipeline owns two of them (ocr_pipe below): the chain of a batch is a sequence of dependent phases, some
// of them latency-bound (det post-processing, cls, the tails of the networks), and two chains side by side on two
// halves of the batch fill each other's gaps.
struct PipeWorker {
  DetStage det;
  // Further detector instances (own stream, network, buffers) for batches of MIXED sizes: every distinct size is its own
  // det pass (a few images at most), a latency-bound chain of ~90 small launches that leaves the chip idle - several
  // chains side by side, each driven by its own host thread, fill it.  OCR_DET_LANES (default 8) instances in all.
  std::vector<std::unique_ptr<DetStage>> det_extra;
  DetConfig det_cfg;
  int det_lanes = 8;
  bool det_ragged = true;  // OCR_DET_RAGGED=0: mixed-size batches as one detector pass per distinct size (rounds 1-2)
  bool det_post_ragged = true;  // OCR_DET_RAGGED=net: ragged network, BoxesFromBitmap per size group on the lanes
  RecStage rec;
  std::unique_ptr<ClsStage> cls;
  DevBuf<RotDesc> rot_desc;
  DevBuf<int> rot_seg;
  int crop_mode = 0;  // OCR_CROP_BOUNDING_RECT | OCR_CROP_ROTATE
  DevBuf<uint8_t> crop_arena;
  DevBuf<WarpDesc> warp_desc;
  std::vector<CropPlan> line_plan;  // OCR_CROP_ROTATE: the crop geometry of every line of the current run
  std::vector<int32_t> boxes;  // [image in layout order][cap][8]
  std::vector<int> nbox;
  static constexpr int kCap = 1000;  // max_candidates bounds the boxes of one image (postprocess_op.cpp:260)

  int create(const DetConfig& d, const RecConfig& r, const ClsConfig* k, int crop, std::string& err) {
    int code = 0;
    if (!det.create(d, err, code)) return code ? code : OCR_ERR_DEVICE;
    det_cfg = d;
    if (!rec.create(r, err, code)) return code ? code : OCR_ERR_DEVICE;
    rec.want_taps = false;
    if (k) {
      cls.reset(new ClsStage());
      if (!cls->create(*k, err, code)) return code ? code : OCR_ERR_DEVICE;
    }
    crop_mode = crop;
    return OCR_OK;
  }

  // a further detector instance; it takes over the timing state of the pipeline (ocr_pipe_timing[_filter]) so that the
  // per-kernel survey sees the chunks that run on it
  bool timing_on = false;
  std::string timing_filter;
  int add_det_extra(std::string& err) {
    std::unique_ptr<DetStage> d(new DetStage());
    int code = 0;
    if (!d->create(det_cfg, err, code)) return code ? code : OCR_ERR_DEVICE;
    d->net().set_timing_filter(timing_filter);
    d->net().enable_timing(timing_on);
    det_extra.push_back(std::move(d));
    return OCR_OK;
  }

  // What the phases of one run_images call share: the batch (or a chain's part of it), its text lines and what was read in them
  struct Run {
    uint8_t* base;
    const std::vector<StageSlot::Img>& imgs;
    const std::vector<StageSlot::Group>& groups;
    const float* probs;
    double* times;  // det | crops + cls | rec
    std::string& err;
    double t_last = now_ms();
    void lap(int k) { const double t = now_ms(); times[k] += t - t_last; t_last = t; }
    std::vector<LineSrc> lines;
    std::vector<int> seg{0};    // lines seg[i] .. seg[i + 1] are image i's
    std::vector<int> line_box;  // box index (within its image) of every line
    std::vector<int> labels;    // per line: 1 = the classifier turned the crop by 180 degrees
    static constexpr int max_len = 256;
    std::vector<int32_t> ids, lens, csteps, cnsteps, geom;  // the recognizer's answers per line (ids, csteps, cnsteps, cprobs: x max_len)
    std::vector<float> scores, cprobs;
  };
  int32_t* boxes_of(size_t img) { return boxes.data() + img * kCap * 8; }

  // ---- run: det per size group, then ONE cls pass and ONE rec pass over the crops of every image of the batch
  // (results are batch-invariant, so pooling lines across sizes changes nothing but the launch count)
  int run_images(uint8_t* base, const std::vector<StageSlot::Img>& imgs, const std::vector<StageSlot::Group>& groups, const float* probs,
                 WordLists& out_words, IdLists& out_ids, double times[3], std::string& err, CharLists* out_chars = nullptr) {
    const size_t count = imgs.size();
    boxes.resize(count * kCap * 8);
    nbox.assign(count, 0);
    Run r{base, imgs, groups, probs, times, err};
    if (int rc = detect(r)) return rc;
    r.lap(0);
    if (int rc = crop_lines(r)) return rc;
    out_words.assign(count, {}); out_ids.assign(count, {});
    if (out_chars) out_chars->assign(count, {});
    if (r.lines.empty()) return OCR_OK;
    if (int rc = classify_and_turn(r)) return rc;
    r.lap(1);
    if (int rc = recognize(r, out_chars != nullptr)) return rc;
    r.lap(2);
    collect(r, out_words, out_ids, out_chars);
    return OCR_OK;
  }

  int detect(Run& r) {
    // A server detector (arch.txt: srv_det) has no ragged launch list (DetStage::mixed_net refuses it) and never gets a
    // further instance: each one would load, bind and tune another ResNet50.  Its size groups run one after another on
    // the chain's one detector, whatever OCR_DET_RAGGED and OCR_DET_LANES say.
    const bool srv_det = det.srv() != nullptr;
    const int lanes = srv_det ? 1 : (int)std::min<size_t>((size_t)det_lanes, r.groups.size());
    if (r.groups.size() > 1 && det_ragged && !srv_det) return detect_ragged(r, lanes);
    return lanes <= 1 ? detect_serial(r) : detect_lanes(r, lanes);
  }
  int det_group(Run& r, DetStage& d, const StageSlot::Group& g, std::string& e) {  // one size group: one detector pass
    const size_t row = (size_t)g.cols * 3, img_bytes = row * g.rows;
    return d.run_device(r.base + g.off, img_bytes, row, g.rows, g.cols, g.count, boxes_of(g.first), kCap, nbox.data() + g.first, nullptr, e,
                        r.probs ? r.probs + g.prob_off : nullptr);
  }
  int detect_serial(Run& r) {
    for (const auto& g : r.groups)
      if (int rc = det_group(r, det, g, r.err)) return rc;
    return OCR_OK;
  }
  int detect_lanes(Run& r, int lanes) {  // OCR_DET_RAGGED=0: size group gi on detector instance gi % lanes, a host thread per instance
    while ((int)det_extra.size() < lanes - 1)   // created on first use: single-size callers never pay for them
      if (int rc = add_det_extra(r.err)) return rc;
    // the clone was enqueued on lane 0's stream: the other lanes' streams must not read it earlier
    if (g_stream_sync(det.stream()) != hipSuccess) { r.err = "det stream sync failed"; return OCR_ERR_DEVICE; }
    return run_side_by_side(lanes, r.err, [&](int l, std::string& e) -> int {
      DetStage& d = l == 0 ? det : *det_extra[l - 1];
      for (size_t gi = l; gi < r.groups.size(); gi += lanes)
        if (int rc = det_group(r, d, r.groups[gi], e)) return rc;
      return OCR_OK;
    });
  }
  // MIXED sizes (round 3): ONE detector network pass over all size groups (every image keeps its own size inside a
  // ragged launch: Net::run_ragged_images) instead of a latency-bound pass per distinct size.  Chunks bound the activation
  // arena (~64 Mpixel of detector input per launch, what a uniform batch of 64 x 960 x 960 needs).
  int detect_ragged(Run& r, int lanes) {
    const auto& groups = r.groups;
    std::vector<DetStage::MixedGroup> mg(groups.size());
    std::vector<size_t> gpx(groups.size());
    for (size_t gi = 0; gi < groups.size(); ++gi) {
      const auto& g = groups[gi];
      mg[gi] = DetStage::MixedGroup{g.rows, g.cols, g.count, g.off, g.prob_off};
      gpx[gi] = (size_t)g.count * pipe_plan::det_pixels(g.rows, g.cols, det.cfg().limit_type, det.cfg().limit_side_len);
    }
    static const size_t budget = [] { const char* e = getenv("OCR_DET_CHUNK_MP"); return (size_t)(e && atoi(e) > 0 ? atoi(e) : 64) << 20; }();
    const std::vector<std::pair<size_t, size_t>> chunks = pipe_plan::det_chunks(gpx, budget);
    // Two network instances whenever there is more than one chunk - whatever OCR_DET_LANES says (the lanes only deal
    // the per-group post-processing of the OCR_DET_RAGGED=net / dilation branch): chunk k+1's network is enqueued (own
    // arena, own maps) BEFORE chunk k's maps are post-processed, so that the latency-bound post of one chunk runs under the
    // dense kernels of the next - and so it must not run on the instance that holds them.
    const int want_extra = std::max(lanes - 1, chunks.size() > 1 ? 1 : 0);
    while ((int)det_extra.size() < want_extra)
      if (int rc = add_det_extra(r.err)) return rc;
    auto net_stage = [&](size_t k) -> DetStage& { return (k & 1) && !det_extra.empty() ? *det_extra[0] : det; };
    auto start = [&](size_t k) {
      return net_stage(k).mixed_net(r.base, mg.data() + chunks[k].first, (int)(chunks[k].second - chunks[k].first), r.probs, r.err);
    };
    if (int rc = start(0)) return rc;
    for (size_t k = 0; k < chunks.size(); ++k) {
      const size_t g0 = chunks[k].first, g1 = chunks[k].second;
      DetStage& src = net_stage(k);
      const bool more = k + 1 < chunks.size();
      // the next chunk's stage has finished ITS previous chunk's post work (it was a lane two chunks ago: joined)
      if (more)
        if (int rc = start(k + 1)) return rc;
      if (!det.cfg().use_dilation && det_post_ragged) {
        // every image of the chunk through ONE pass of the post-processing kernels (each takes its image's own map
        // size), on the stage that ran the chunk's network; it ends with a stream synchronisation
        const int first = groups[g0].first;
        if (int rc = src.post_mixed(mg.data() + g0, (int)(g1 - g0), boxes_of(first), kCap, nbox.data() + first, r.err)) return rc;
      } else {
        if (int rc = post_on_lanes(r, mg, g0, g1, src, more ? &net_stage(k + 1) : nullptr)) return rc;
        // this chunk's maps are free again once its network stage is idle (its own post lane, if any, has synchronised;
        // when it was not a post lane the network pass itself must be over before the stage takes chunk k+2)
        if (g_stream_sync(src.stream()) != hipSuccess) { r.err = "det stream sync failed"; return OCR_ERR_DEVICE; }
      }
      src.collect_timings();
    }
    return OCR_OK;
  }
  // BoxesFromBitmap of the groups [g0, g1) of a chunk whose network ran on `src`, group by group, dealt over every detector
  // instance but `busy` (its stream is taken by the next chunk's network), a host thread per instance
  int post_on_lanes(Run& r, const std::vector<DetStage::MixedGroup>& mg, size_t g0, size_t g1, DetStage& src, DetStage* busy) {
    std::vector<DetStage*> post;
    if (&det != busy) post.push_back(&det);
    for (auto& d : det_extra)
      if (d.get() != busy) post.push_back(d.get());
    const int np = (int)post.size();
    return run_side_by_side(np, r.err, [&](int l, std::string& e) -> int {
      DetStage& d = *post[l];
      for (size_t gi = g0 + l; gi < g1; gi += np) {
        const auto& g = r.groups[gi];
        if (int rc = d.post_group(src.mixed_prob((int)(gi - g0)), src.mixed_bitmap((int)(gi - g0)), mg[gi], &d == &src ? nullptr : src.done(),
                                  boxes_of(g.first), kCap, nbox.data() + g.first, e))
          return rc;
      }
      return OCR_OK;
    });
  }

  // the text lines of every image: cv::boundingRect(points) & image rect (ocr_worker.cpp:245-258), or rotate_crops
  int crop_lines(Run& r) {
    line_plan.clear();
    if (crop_mode == OCR_CROP_ROTATE) return rotate_crops(r.base, r.imgs, r.lines, r.seg, r.line_box, r.err);
    std::vector<pipe_plan::RectLine> rl;
    for (size_t i = 0; i < r.imgs.size(); ++i) {
      const StageSlot::Img& im = r.imgs[i];
      pipe_plan::rect_lines(boxes_of(i), nbox[i], im.rows, im.cols, rl);
      for (const auto& l : rl) {
        r.line_box.push_back(l.box);
        r.lines.push_back(LineSrc{r.base + im.off, (size_t)im.cols * 3, l.x, l.y, l.w, l.h});
      }
      r.seg.push_back((int)r.lines.size());
    }
    return OCR_OK;
  }

  int classify_and_turn(Run& r) {
    if (!cls) return OCR_OK;
    r.labels.resize(r.lines.size());
    std::vector<float> scores(r.lines.size());
    if (int rc = cls->run_lines(r.lines, r.labels.data(), scores.data(), r.err)) return rc;
    // rotate in request order, in place on the device copy (cv::rotate on ROI views aliasing the image)
    std::vector<RotDesc> rd;
    for (size_t k = 0; k < r.lines.size(); ++k) {
      const LineSrc& L = r.lines[k];
      if (r.labels[k] == 1) rd.push_back(RotDesc{const_cast<uint8_t*>(L.img), L.stride, L.x, L.y, L.w, L.h});
    }
    if (int rc = rotate180_in_order(rd, rot_desc, rot_seg, cls->stream(), r.err)) return rc;
    if (g_stream_sync(cls->stream()) != hipSuccess) { r.err = "cls stream sync failed"; return OCR_ERR_DEVICE; }
    return OCR_OK;
  }

  int recognize(Run& r, bool chars) {
    const size_t n = r.lines.size();
    r.ids.resize(n * Run::max_len); r.lens.resize(n); r.scores.resize(n);
    if (!chars) return rec.run_lines(r.lines, r.seg, r.ids.data(), Run::max_len, r.lens.data(), r.scores.data(), r.err);
    r.csteps.resize(r.ids.size()); r.cnsteps.resize(r.ids.size()); r.cprobs.resize(r.ids.size()); r.geom.resize(n * 3);
    RecStage::CharOut co;
    co.steps = r.csteps.data(); co.nsteps = r.cnsteps.data(); co.probs = r.cprobs.data(); co.geom = r.geom.data();
    return rec.run_lines_chars(r.lines, r.seg, r.ids.data(), Run::max_len, r.lens.data(), r.scores.data(), co, r.err);
  }

  // words, class ids and (out_chars) character quads per image
  void collect(const Run& r, WordLists& out_words, IdLists& out_ids, CharLists* out_chars) {
    for (size_t i = 0; i < r.imgs.size(); ++i) {
      for (int k = r.seg[i]; k < r.seg[i + 1]; ++k) {
        const size_t at = (size_t)k * Run::max_len;
        ocr_word w;
        memcpy(w.box, boxes_of(i) + (size_t)r.line_box[k] * 8, sizeof(w.box));
        w.ids_off = (int32_t)out_ids[i].size();
        w.ids_len = r.lens[k];
        w.confidence = r.scores[k];
        out_ids[i].insert(out_ids[i].end(), r.ids.begin() + at, r.ids.begin() + at + r.lens[k]);
        out_words[i].push_back(w);
        for (int j = 0; out_chars && j < r.lens[k]; ++j) {  // the character's quad from the line's own geometry (crop.h, char_quad)
          ocr_char ch;
          ch.step = r.csteps[at + j]; ch.nsteps = r.cnsteps[at + j]; ch.prob = r.cprobs[at + j];
          const LineSrc& L = r.lines[k];
          char_quad(ch.step, ch.nsteps, r.geom[3 * k], r.geom[3 * k + 1], r.geom[3 * k + 2], L.w, L.h, !r.labels.empty() && r.labels[k] == 1,
                    crop_mode == OCR_CROP_ROTATE ? &line_plan[k] : nullptr, L.x, L.y, r.imgs[i].rows, r.imgs[i].cols, ch.quad);
          (*out_chars)[i].push_back(ch);
        }
      }
    }
  }

  // crop_mode OCR_CROP_ROTATE: every box becomes its own perspective-rectified image
  // (Utility::GetRotateCropImage, utility.cpp:137-190) in the crop arena
  int rotate_crops(const uint8_t* base, const std::vector<StageSlot::Img>& imgs, std::vector<LineSrc>& lines, std::vector<int>& seg,
                   std::vector<int>& line_box, std::string& err) {
    std::vector<WarpDesc> wd;
    std::vector<size_t> off;
    size_t total = 0;
    int max_px = 0;
    for (int i = 0; i < (int)imgs.size(); ++i) {
      const int rows = imgs[i].rows, cols = imgs[i].cols;
      const size_t row = (size_t)cols * 3;
      for (int j = 0; j < nbox[i]; ++j) {
        CropPlan p;
        if (!plan_rotate_crop(rows, cols, &boxes[((size_t)i * kCap + j) * 8], p)) continue;
        WarpDesc d;
        d.src = base + imgs[i].off + (size_t)p.top * row + (size_t)p.left * 3;
        d.sstride = row; d.sw = p.sw; d.sh = p.sh; d.dst = nullptr; d.dw = p.dw; d.dh = p.dh; d.rot = p.rot; d.bw0 = p.bw0;
        memcpy(d.m, p.minv, sizeof(d.m));
        wd.push_back(d);
        off.push_back(total);
        total += ((size_t)p.dw * p.dh * 3 + 15) & ~(size_t)15;
        max_px = std::max(max_px, p.dw * p.dh);
        line_box.push_back(j);
        line_plan.push_back(p);
        lines.push_back(LineSrc{nullptr, (size_t)p.ocols * 3, 0, 0, p.ocols, p.orows});
      }
      seg.push_back((int)lines.size());
    }
    if (wd.empty()) return OCR_OK;
    if (!crop_arena.ensure(total, err) || !warp_desc.ensure(wd.size(), err)) return OCR_ERR_DEVICE;
    for (size_t k = 0; k < wd.size(); ++k) {
      wd[k].dst = crop_arena.p + off[k];
      lines[k].img = wd[k].dst;
    }
    if (hipMemcpyAsync(warp_desc.p, wd.data(), wd.size() * sizeof(WarpDesc), hipMemcpyHostToDevice, det.stream()) != hipSuccess) {
      err = "crop list upload failed";
      return OCR_ERR_DEVICE;
    }
    launch_warp_crops(warp_desc.p, (int)wd.size(), max_px, det.stream());
    if (g_stream_sync(det.stream()) != hipSuccess) { err = "crop kernel failed"; return OCR_ERR_DEVICE; }
    return OCR_OK;
  }
};

struct ocr_pipe {
  PipeWorker w0;
  // The second chain (OCR_PIPE_PHASES / ocr_pipe_cfg.phases = 2, the default): a batch of two or more images is cut in
  // two parts that run concurrently, each on its own worker and host thread.  Results are per image and do not depend
  // on what else is in a batch, so nothing changes but the overlap.  phases = 1 keeps one chain (one kernel at a time
  // owns the chip: what the per-kernel roofline figures of bench.py are measured with).
  std::vector<std::unique_ptr<PipeWorker>> extra;  // chains 2 .. phases
  int phases = 2;
  int device = 0;
  StageSlot slots[2];
  hipStream_t copy_stream = nullptr;
  FrameScratch frame_scratch;
  DevBuf<uint8_t> work;  // the requests' clones (OCRRequest copies the Mat, ocr_worker.h:28-29): cls rotates in place on them
  // Two batches in flight (round 5, ocr_pipe_run_device_on / ocr_pipe_run_staged_on): a call that names a chain runs its WHOLE
  // batch on that chain's worker, with a clone buffer of the chain's own; calls on different chains may run concurrently from
  // different host threads - chain 0 on batch k while chain 1 is on batch k+1 - so that consecutive batches overlap instead of
  // the two halves of one (no join per batch: what two free-running handles gained over one, without the second handle)
  DevBuf<uint8_t> work_chain[4];
  PipeWorker* worker(int c) { return c == 0 ? &w0 : (c >= 1 && c <= (int)extra.size() ? extra[c - 1].get() : nullptr); }
  std::vector<PipeWorker*> workers() {  // every chain's
    std::vector<PipeWorker*> ws{&w0};
    for (auto& w : extra) ws.push_back(w.get());
    return ws;
  }

  ~ocr_pipe() { if (copy_stream) (void)hipStreamDestroy(copy_stream); }

  // ---- stage: a slot takes the layout of a new batch (pipe_plan::layout) once its last upload has left the pinned buffer
  int layout(StageSlot& S, int count, const std::function<void(int, int&, int&)>& size_of, std::string& err) {
    if (!copy_stream && hipStreamCreateWithFlags(&copy_stream, hipStreamNonBlocking) != hipSuccess) { err = "hipStreamCreate failed"; return OCR_ERR_DEVICE; }
    if (!S.ready && hipEventCreateWithFlags(&S.ready, hipEventDisableTiming) != hipSuccess) { err = "hipEventCreate failed"; return OCR_ERR_DEVICE; }
    if (S.staged && hipEventSynchronize(S.ready) != hipSuccess) { err = "staging event failed"; return OCR_ERR_DEVICE; }  // pinned buffer free again
    // from here to the end of stage() / stage_coded() the slot holds a half-written batch: a failure on the way must not
    // leave it runnable (a later ocr_pipe_run_staged would run the new layout over stale pixels)
    S.staged = false;
    std::vector<std::pair<int, int>> sizes(count);
    for (int i = 0; i < count; ++i) size_of(i, sizes[i].first, sizes[i].second);
    pipe_plan::Layout L = pipe_plan::layout(sizes, w0.det.cfg().limit_type, w0.det.cfg().limit_side_len);
    // probability maps attached to the slot (benchmark protocol) stay valid only while the layout is the same
    if (!pipe_plan::same_layout(S.imgs, L.imgs)) S.has_probs = false;
    S.imgs = std::move(L.imgs); S.groups = std::move(L.groups);
    S.bytes = L.bytes; S.prob_floats = L.prob_floats;
    if (!S.dev.ensure(S.bytes + 256, err)) return OCR_ERR_DEVICE;
    return OCR_OK;
  }

  // ---- stage: host images -> pinned -> device (asynchronous after the host copies)
  int stage(int si, const ocr_img* imgs, int count, std::string& err) {
    StageSlot& S = slots[si];
    int rc = layout(S, count, [&](int i, int& r, int& c) { r = imgs[i].rows; c = imgs[i].cols; }, err);
    if (rc) return rc;
    const size_t off = S.bytes;
    if (!S.pinned.reserve(off, err)) return OCR_ERR_DEVICE;
    parallel_copy((size_t)count, off, [&](size_t k) {
      const ocr_img& im = imgs[S.imgs[k].orig];
      const size_t row = (size_t)im.cols * 3, stride = im.row_stride ? im.row_stride : row;
      uint8_t* dst = S.pinned.p + S.imgs[k].off;
      if (stride == row) memcpy(dst, im.data, row * im.rows);
      else for (int y = 0; y < im.rows; ++y) memcpy(dst + row * y, im.data + stride * y, row);
    });
    if (hipMemcpyAsync(S.dev.p, S.pinned.p, off, hipMemcpyHostToDevice, copy_stream) != hipSuccess) { err = "H2D copy failed"; return OCR_ERR_DEVICE; }
    if (hipEventRecord(S.ready, copy_stream) != hipSuccess) { err = "hipEventRecord failed"; return OCR_ERR_DEVICE; }
    S.staged = true;
    return OCR_OK;
  }

  // ---- stage a batch of tagged frame descriptors, of any kinds in any mix: the frames of a kind are decoded by that kind's
  // row of kFrameKinds, on the copy stream, into the slot.  The caller has validated every frame (a known kind, a sound
  // descriptor) before the sizes are used: a batch refused there leaves the slot as it was.
  int stage_coded(int si, const ocr_coded_frame* frames, int count, std::string& err) {
    StageSlot& S = slots[si];
    int rc = layout(S, count, [&](int i, int& r, int& c) { kFrameKinds[frames[i].kind].size(frames[i].frame, r, c); }, err);
    if (rc) return rc;
    struct Bucket {
      std::vector<const void*> frames;
      std::vector<uint8_t*> dst;
      std::vector<int> ids;  // a frame's place in the batch: what a refusal names
    } bucket[kFrameKindCount];
    for (const StageSlot::Img& im : S.imgs) {
      Bucket& b = bucket[frames[im.orig].kind];
      b.frames.push_back(frames[im.orig].frame);
      b.dst.push_back(S.dev.p + im.off);
      b.ids.push_back(im.orig);
    }
    for (int kind : kFrameLaunchOrder) {
      const Bucket& b = bucket[kind];
      if (b.frames.empty()) continue;
      rc = kFrameKinds[kind].decode(b.frames.data(), (int)b.frames.size(), b.dst.data(), frame_scratch, copy_stream, err, b.ids.data());
      if (rc) return rc;
    }
    if (hipEventRecord(S.ready, copy_stream) != hipSuccess) { err = "hipEventRecord failed"; return OCR_ERR_DEVICE; }
    S.staged = true;
    return OCR_OK;
  }

  // benchmark protocol for synthetic weights: per staged image a probability map of the
  // detector's input resolution that replaces the network's map for thresholding / scoring
  int slot_probs(int si, const float* const* probs, int count, std::string& err) {
    StageSlot& S = slots[si];
    if (!S.staged || count != (int)S.imgs.size()) { err = "stage the slot's images first (same count)"; return OCR_ERR_ARG; }
    if (!S.probs.ensure(S.prob_floats + 64, err)) return OCR_ERR_DEVICE;
    for (int k = 0; k < count; ++k) {
      const size_t n = (k + 1 < count ? S.imgs[k + 1].prob_off : S.prob_floats) - S.imgs[k].prob_off;
      const hipError_t e = hipMemcpyAsync(S.probs.p + S.imgs[k].prob_off, probs[S.imgs[k].orig], n * sizeof(float), hipMemcpyDefault, copy_stream);
      if (e != hipSuccess) {
        err = std::string("probability map upload failed: ") + hipGetErrorString(e);
        return OCR_ERR_DEVICE;
      }
    }
    if (hipEventRecord(S.ready, copy_stream) != hipSuccess) { err = "hipEventRecord failed"; return OCR_ERR_DEVICE; }
    S.has_probs = true;
    return OCR_OK;
  }

  // ---- run: one chain, or several chains on as many parts of the batch (pipe_plan::split), each on its own host thread
  int run_images(uint8_t* base, const std::vector<StageSlot::Img>& imgs, const std::vector<StageSlot::Group>& groups, const float* probs,
                 WordLists& out_words, IdLists& out_ids, double times[3], std::string& err, CharLists* out_chars = nullptr) {
    const size_t count = imgs.size();
    const int K = (int)std::min(1 + extra.size(), count);
    if (K < 2) return w0.run_images(base, imgs, groups, probs, out_words, out_ids, times, err, out_chars);
    const std::vector<pipe_plan::Part> parts = pipe_plan::split(imgs, groups, K, w0.det.cfg().limit_type, w0.det.cfg().limit_side_len);
    // the clone was enqueued on worker 0's detector stream: the other workers' streams must not read it earlier
    if (g_stream_sync(w0.det.stream()) != hipSuccess) { err = "det stream sync failed"; return OCR_ERR_DEVICE; }
    std::vector<WordLists> W(K); std::vector<IdLists> I(K); std::vector<CharLists> Ch(K);
    std::vector<std::array<double, 3>> t(K, std::array<double, 3>{0, 0, 0});
    // (round 5: starting chain c a few milliseconds late - 3 .. 24 ms - so that one chain's matrix-bound kernels meet the other's
    // HBM-bound ones costs 2-11 %: 1282 -> 1257 / 1218 / 1177 / 1155 / 1140 img/s; what two free-running handles gain comes from
    // batches overlapping batches, not from a phase offset inside one)
    const int rc = run_side_by_side(K, err, [&](int c, std::string& e) -> int {  // part c on worker c
      if (c) (void)rt_set_device(device);
      if (parts[c].imgs.empty()) return OCR_OK;
      return worker(c)->run_images(base, parts[c].imgs, parts[c].groups, probs, W[c], I[c], t[c].data(), e, out_chars ? &Ch[c] : nullptr);
    });
    if (rc) return rc;
    out_words.assign(count, {}); out_ids.assign(count, {});
    if (out_chars) out_chars->assign(count, {});
    for (int p = 0; p < K; ++p)
      for (size_t k = 0; k < parts[p].index.size(); ++k) {
        out_words[parts[p].index[k]] = std::move(W[p][k]);
        out_ids[parts[p].index[k]] = std::move(I[p][k]);
        if (out_chars) (*out_chars)[parts[p].index[k]] = std::move(Ch[p][k]);
      }
    for (int k = 0; k < 3; ++k) {  // the chains ran side by side: per stage, the busiest chain's time
      double m = 0;
      for (int c = 0; c < K; ++c) m = std::max(m, t[c][k]);
      times[k] += m;
    }
    return OCR_OK;
  }

  struct Out {  // the caller's result arrays (ocr_pipe_run*); times and chars may be null
    ocr_word* words; int cap_words; int* word_off; int* nwords; int32_t* ids; int cap_ids; double* times; ocr_char* chars;
  };
  // The tail of every run entry point.  The batch's clone (OCRRequest copies the Mat, ocr_worker.h:28-29: cls rotates in place
  // on it) is enqueued, behind `after` if there is one, on the detector stream of the chain that runs it; the batch runs whole
  // on one chain (chain >= 0: two batches in flight) or split over all; image i of the caller is imgs[order[i]].
  int clone_run_emit(int chain, const void* src, size_t bytes, hipEvent_t after, const std::vector<StageSlot::Img>& imgs,
                     const std::vector<StageSlot::Group>& groups, const float* probs, const std::vector<int>& order, const Out& o) {
    PipeWorker* one = chain >= 0 ? worker(chain) : nullptr;
    if (chain >= 0 && !one) return fail(OCR_ERR_ARG, "no such chain (0 <= chain < phases)");
    PipeWorker& first = one ? *one : w0;
    DevBuf<uint8_t>& clone = one ? work_chain[chain] : work;
    std::string err;
    if (after && hipStreamWaitEvent(first.det.stream(), after, 0) != hipSuccess) return fail(OCR_ERR_DEVICE, "hipStreamWaitEvent failed");
    if (!clone.ensure(bytes + 256, err)) return fail(OCR_ERR_DEVICE, err);
    CAPI_HIP(hipMemcpyAsync(clone.p, src, bytes, hipMemcpyDeviceToDevice, first.det.stream()));
    double t[3] = {0, 0, 0};
    WordLists W; IdLists I; CharLists C;
    CharLists* pc = o.chars ? &C : nullptr;
    const int rc = one ? one->run_images(clone.p, imgs, groups, probs, W, I, t, err, pc) : run_images(clone.p, imgs, groups, probs, W, I, t, err, pc);
    if (rc) return fail(rc, err);
    if (o.times) { o.times[0] = t[0]; o.times[1] = t[1]; o.times[2] = t[2]; }
    if (!pipe_plan::emit(W, I, order, o.words, o.cap_words, o.word_off, o.nwords, o.ids, o.cap_ids, pc, o.chars))
      return fail(OCR_ERR_CAPACITY, "result buffers too small");
    return OCR_OK;
  }

  // run a staged slot: wait for its upload, clone, run, hand the results back in the caller's order
  int run_slot(int si, const Out& o, int chain = -1) {
    StageSlot& S = slots[si];
    if (!S.staged || S.imgs.empty()) return fail(OCR_ERR_ARG, "nothing staged in this slot");
    std::vector<int> order(S.imgs.size());  // order[original index] = layout index
    for (size_t k = 0; k < S.imgs.size(); ++k) order[S.imgs[k].orig] = (int)k;
    return clone_run_emit(chain, S.dev.p, S.bytes, S.ready, S.imgs, S.groups, S.has_probs ? S.probs.p : nullptr, order, o);
  }
};

extern "C" {

void ocr_pipe_cfg_default(ocr_pipe_cfg* c) {
  if (!c) return;
  memset(c, 0, sizeof(*c));
  ocr_det_cfg_default(&c->det);
  ocr_cls_cfg_default(&c->cls);
  ocr_rec_cfg_default(&c->rec);
  c->enable_cls = 0;
  c->crop_mode = OCR_CROP_BOUNDING_RECT;
}

int ocr_pipe_create(const ocr_pipe_cfg* c, ocr_pipe** out) {
  if (!c || !out || !c->det.model_dir || !c->rec.model_dir || !c->rec.label_path) return fail(OCR_ERR_ARG, "null argument");
  if (c->enable_cls && !c->cls.model_dir) return fail(OCR_ERR_ARG, "cls model_dir missing");
  std::unique_ptr<ocr_pipe> h(new ocr_pipe());
  h->device = c->det.device_id;
  if (c->crop_mode != OCR_CROP_BOUNDING_RECT && c->crop_mode != OCR_CROP_ROTATE) return fail(OCR_ERR_ARG, "unknown crop_mode");
  if (c->phases < 0 || c->phases > 4) return fail(OCR_ERR_ARG, "phases must be 0 (default) or 1..4");
  h->phases = c->phases ? c->phases : 2;
  if (const char* e = getenv("OCR_PIPE_PHASES")) h->phases = std::min(4, std::max(1, atoi(e)));
  std::string err;
  DetConfig d;
  d.model_dir = c->det.model_dir; d.device = c->det.device_id;
  if (c->det.limit_type) d.limit_type = c->det.limit_type;
  d.limit_side_len = c->det.limit_side_len; d.thresh = c->det.det_db_thresh; d.box_thresh = c->det.det_db_box_thresh;
  d.unclip_ratio = c->det.det_db_unclip_ratio;
  if (c->det.det_db_score_mode) d.score_mode = c->det.det_db_score_mode;
  d.use_dilation = c->det.use_dilation;
  if (c->det.precision) d.precision = c->det.precision;
  d.max_batch = c->det.max_batch > 0 ? c->det.max_batch : 1;
  d.cv_compat = resolve_cv_compat(c->det.cv_compat);
  RecConfig r;
  r.model_dir = c->rec.model_dir; r.label_path = c->rec.label_path; r.device = c->det.device_id;
  r.batch_num = c->rec.rec_batch_num; r.img_h = c->rec.rec_img_h; r.img_w = c->rec.rec_img_w; r.sort_mode = c->rec.sort_mode;
  if (c->rec.precision) r.precision = c->rec.precision;
  ClsConfig k;
  if (c->enable_cls) {
    k.model_dir = c->cls.model_dir; k.device = c->det.device_id; k.thresh = c->cls.cls_thresh;
    k.batch_num = c->cls.cls_batch_num > 0 ? c->cls.cls_batch_num : 1;
    if (c->cls.precision) k.precision = c->cls.precision;
  }
  int lanes = 8;
  if (const char* e = getenv("OCR_DET_LANES")) lanes = std::min(32, std::max(1, atoi(e)));
  int rc = h->w0.create(d, r, c->enable_cls ? &k : nullptr, c->crop_mode, err);
  if (rc) return fail(rc, err);
  for (int p = 1; p < h->phases; ++p) {
    h->extra.emplace_back(new PipeWorker());
    rc = h->extra.back()->create(d, r, c->enable_cls ? &k : nullptr, c->crop_mode, err);
    if (rc) return fail(rc, err);
  }
  // the detector lanes (mixed-size batches) are dealt over the chains
  const char* ragged = getenv("OCR_DET_RAGGED");
  for (PipeWorker* w : h->workers()) {
    w->det_lanes = std::max(1, (lanes + h->phases - 1) / h->phases);
    if (ragged) { w->det_ragged = ragged[0] != '0'; w->det_post_ragged = ragged[0] != 'n'; }
  }
  // two idle high-priority streams per device (once per process), created after the first pipeline's stage streams and
  // before the detector lanes' (which come into being at the first mixed-size batch): the configuration in which the
  // lanes measured fastest (capi_net.hip)
  priority_anchor(h->device, 2);
  *out = h.release();
  return OCR_OK;
}
void ocr_pipe_destroy(ocr_pipe* h) { delete h; }

static int pipe_run_device(ocr_pipe* h, int chain, const void* dev_bgr, int rows, int cols, int count, const float* dev_prob, ocr_word* words,
                           int cap_words, int* word_off, int* nwords, int32_t* ids, int cap_ids, double times[3]) {
  if (!h || !dev_bgr || rows <= 0 || cols <= 0 || count < 1 || !words || !word_off || !nwords || !ids)
    return fail(OCR_ERR_ARG, "bad argument");
  CAPI_HIP(rt_set_device(h->device));
  const size_t img_bytes = (size_t)rows * cols * 3;
  std::vector<StageSlot::Img> imgs(count);
  std::vector<int> order(count);
  for (int i = 0; i < count; ++i) { imgs[i] = {rows, cols, i, img_bytes * i, 0}; order[i] = i; }
  return h->clone_run_emit(chain, dev_bgr, img_bytes * count, nullptr, imgs, {{rows, cols, 0, count, 0, 0}}, dev_prob, order,
                           {words, cap_words, word_off, nwords, ids, cap_ids, times, nullptr});
}
int ocr_pipe_run_device(ocr_pipe* h, const void* dev_bgr, int rows, int cols, int count, const float* dev_prob, ocr_word* words,
                        int cap_words, int* word_off, int* nwords, int32_t* ids, int cap_ids, double times[3]) {
  return pipe_run_device(h, -1, dev_bgr, rows, cols, count, dev_prob, words, cap_words, word_off, nwords, ids, cap_ids, times);
}
int ocr_pipe_run_device_on(ocr_pipe* h, int chain, const void* dev_bgr, int rows, int cols, int count, const float* dev_prob,
                           ocr_word* words, int cap_words, int* word_off, int* nwords, int32_t* ids, int cap_ids, double times[3]) {
  if (chain < 0) return fail(OCR_ERR_ARG, "no such chain (0 <= chain < phases)");
  return pipe_run_device(h, chain, dev_bgr, rows, cols, count, dev_prob, words, cap_words, word_off, nwords, ids, cap_ids, times);
}

static bool stage_args_ok(const ocr_pipe* h, bool images, int slot, int count) { return h && images && count >= 1 && (slot == 0 || slot == 1); }

// the tail of the five entry points below: every frame has been validated
static int stage_validated(ocr_pipe* h, int slot, const std::vector<ocr_coded_frame>& frames) {
  CAPI_HIP(rt_set_device(h->device));
  std::string err;
  const int rc = h->stage_coded(slot, frames.data(), (int)frames.size(), err);
  return rc ? fail(rc, err) : OCR_OK;
}
static std::vector<ocr_coded_frame> tagged(const ocr_jpeg_frame* frames, int count) {
  std::vector<ocr_coded_frame> t((size_t)count);
  for (int i = 0; i < count; ++i) t[i] = ocr_coded_frame{OCR_FRAME_JPEG, frames + i};
  return t;
}

int ocr_pipe_stage(ocr_pipe* h, int slot, const ocr_img* imgs, int count) {
  if (!stage_args_ok(h, imgs, slot, count)) return fail(OCR_ERR_ARG, "bad argument");
  for (int i = 0; i < count; ++i)
    if (!imgs[i].data || imgs[i].rows <= 0 || imgs[i].cols <= 0) return fail(OCR_ERR_ARG, "Empty image data provided");
  CAPI_HIP(rt_set_device(h->device));
  std::string err;
  const int rc = h->stage(slot, imgs, count, err);
  return rc ? fail(rc, err) : OCR_OK;
}

int ocr_pipe_stage_jpeg(ocr_pipe* h, int slot, const ocr_jpeg_img* imgs, int count) {
  if (!stage_args_ok(h, imgs, slot, count)) return fail(OCR_ERR_ARG, "bad argument");
  for (int i = 0; i < count; ++i)
    if (!jpeg_img_valid(imgs[i])) return fail(OCR_ERR_ARG, "bad JPEG coefficient descriptor");
  std::vector<ocr_jpeg_frame> frames((size_t)count);
  for (int i = 0; i < count; ++i) {
    frames[i] = jpeg_frame_of(imgs[i]);
    if (const char* fault = jpeg_frame_fault(frames[i])) return fail(OCR_ERR_ARG, fault);
  }
  return stage_validated(h, slot, tagged(frames.data(), count));
}

int ocr_pipe_stage_jpeg_frames(ocr_pipe* h, int slot, const ocr_jpeg_frame* frames, int count) {
  if (!stage_args_ok(h, frames, slot, count)) return fail(OCR_ERR_ARG, "bad argument");
  for (int i = 0; i < count; ++i)
    if (const char* fault = jpeg_frame_fault(frames[i])) return fail(OCR_ERR_ARG, fault);
  return stage_validated(h, slot, tagged(frames, count));
}

int ocr_pipe_stage_frames(ocr_pipe* h, int slot, const ocr_jpeg_frame* const* jpegs, const ocr_png_frame* const* pngs,
                          const ocr_raw_frame* const* raws, int count) {
  if (!stage_args_ok(h, jpegs || pngs || raws, slot, count)) return fail(OCR_ERR_ARG, "bad argument");
  std::vector<ocr_coded_frame> t((size_t)count);
  for (int i = 0; i < count; ++i) {
    const ocr_jpeg_frame* j = jpegs ? jpegs[i] : nullptr;
    const ocr_png_frame* p = pngs ? pngs[i] : nullptr;
    const ocr_raw_frame* r = raws ? raws[i] : nullptr;
    if ((j != nullptr) + (p != nullptr) + (r != nullptr) != 1)
      return fail(OCR_ERR_ARG, raws ? "every image is a JPEG frame, a PNG frame or a raw frame: exactly one of the three"
                                    : "every image is a JPEG frame or a PNG frame, not both and not neither");
    if (const char* fault = j ? jpeg_frame_fault(*j) : p ? png_frame_fault(*p) : raw_frame_fault(*r)) return fail(OCR_ERR_ARG, fault);
    t[i] = j ? ocr_coded_frame{OCR_FRAME_JPEG, j} : p ? ocr_coded_frame{OCR_FRAME_PNG, p} : ocr_coded_frame{OCR_FRAME_RAW, r};
  }
  return stage_validated(h, slot, t);
}

int ocr_pipe_stage_batch(ocr_pipe* h, int slot, const ocr_coded_frame* frames, int count) {
  if (!stage_args_ok(h, frames, slot, count)) return fail(OCR_ERR_ARG, "bad argument");
  for (int i = 0; i < count; ++i) {
    const void* f = frames[i].frame;
    if (!f) return fail(OCR_ERR_ARG, "null frame in the batch");
    const int kind = frames[i].kind;
    const char* fault = kind >= 0 && kind < kFrameKindCount ? kFrameKinds[kind].fault(f) : "frame kind is not an ocr_frame_kind";
    if (fault) return fail(OCR_ERR_ARG, fault);
  }
  return stage_validated(h, slot, std::vector<ocr_coded_frame>(frames, frames + count));
}

int ocr_pipe_stage_coded(ocr_pipe* h, int slot, const ocr_jpeg_frame* const* jpegs, const ocr_png_frame* const* pngs, int count) {
  return ocr_pipe_stage_frames(h, slot, jpegs, pngs, nullptr, count);
}

int ocr_pipe_slot_image(ocr_pipe* h, int slot, int index, uint8_t* bgr, size_t cap, int* rows, int* cols) {
  if (!h || !bgr || !rows || !cols || slot < 0 || slot > 1) return fail(OCR_ERR_ARG, "bad argument");
  StageSlot& S = h->slots[slot];
  if (!S.staged) return fail(OCR_ERR_ARG, "nothing is staged in the slot");
  for (const StageSlot::Img& im : S.imgs) {
    if (im.orig != index) continue;
    const size_t bytes = (size_t)im.rows * im.cols * 3;
    if (bytes > cap) return fail(OCR_ERR_CAPACITY, "output buffer too small");
    CAPI_HIP(rt_set_device(h->device));
    CAPI_HIP(hipEventSynchronize(S.ready));
    CAPI_HIP(g_memcpy(bgr, S.dev.p + im.off, bytes, hipMemcpyDeviceToHost));
    *rows = im.rows; *cols = im.cols;
    return OCR_OK;
  }
  return fail(OCR_ERR_ARG, "no staged image with that index");
}

int ocr_pipe_slot_probs(ocr_pipe* h, int slot, const float* const* probs, int count) {
  if (!h || !probs || count < 1 || slot < 0 || slot > 1) return fail(OCR_ERR_ARG, "bad argument");
  for (int i = 0; i < count; ++i) if (!probs[i]) return fail(OCR_ERR_ARG, "null probability map");
  CAPI_HIP(rt_set_device(h->device));
  std::string err;
  const int rc = h->slot_probs(slot, probs, count, err);
  return rc ? fail(rc, err) : OCR_OK;
}

int ocr_pipe_run_staged(ocr_pipe* h, int slot, ocr_word* words, int cap_words, int* word_off, int* nwords, int32_t* ids,
                        int cap_ids, double times[3]) {
  if (!h || slot < 0 || slot > 1 || !words || !word_off || !nwords || !ids) return fail(OCR_ERR_ARG, "bad argument");
  CAPI_HIP(rt_set_device(h->device));
  return h->run_slot(slot, {words, cap_words, word_off, nwords, ids, cap_ids, times, nullptr});
}

int ocr_pipe_run_staged_on(ocr_pipe* h, int chain, int slot, ocr_word* words, int cap_words, int* word_off, int* nwords, int32_t* ids,
                           int cap_ids, double times[3]) {
  if (!h || chain < 0 || slot < 0 || slot > 1 || !words || !word_off || !nwords || !ids) return fail(OCR_ERR_ARG, "bad argument");
  CAPI_HIP(rt_set_device(h->device));
  return h->run_slot(slot, {words, cap_words, word_off, nwords, ids, cap_ids, times, nullptr}, chain);
}

int ocr_pipe_run(ocr_pipe* h, const ocr_img* imgs, int count, ocr_word* words, int cap_words, int* word_off, int* nwords,
                 int32_t* ids, int cap_ids, double times[3]) {
  if (!h || !imgs || count < 1 || !words || !word_off || !nwords || !ids) return fail(OCR_ERR_ARG, "bad argument");
  const int rc = ocr_pipe_stage(h, 0, imgs, count);
  if (rc) return rc;
  return h->run_slot(0, {words, cap_words, word_off, nwords, ids, cap_ids, times, nullptr});
}

int ocr_pipe_run_chars(ocr_pipe* h, const ocr_img* imgs, int count, ocr_word* words, int cap_words, int* word_off, int* nwords,
                       int32_t* ids, int cap_ids, ocr_char* chars, double times[3]) {
  if (!h || !imgs || count < 1 || !words || !word_off || !nwords || !ids || !chars) return fail(OCR_ERR_ARG, "bad argument");
  const int rc = ocr_pipe_stage(h, 0, imgs, count);
  if (rc) return rc;
  return h->run_slot(0, {words, cap_words, word_off, nwords, ids, cap_ids, times, chars});
}

const char* ocr_pipe_label(ocr_pipe* h, int id) {
  if (!h || id < 0 || id >= (int)h->w0.rec.labels().size()) return nullptr;
  return h->w0.rec.labels()[id].c_str();
}

int ocr_pipe_det_shape(ocr_pipe* h, int rows, int cols, int* net_rows, int* net_cols) {
  if (!h || !net_rows || !net_cols) return fail(OCR_ERR_ARG, "null argument");
  float a, b;
  DetStage::resize_shape(rows, cols, h->w0.det.cfg().limit_type, h->w0.det.cfg().limit_side_len, *net_rows, *net_cols, a, b);
  return OCR_OK;
}

static std::vector<Net*> pipe_nets(ocr_pipe* h) {
  std::vector<Net*> v;
  for (PipeWorker* w : h->workers()) {
    v.push_back(&w->det.net());
    for (auto& d : w->det_extra) v.push_back(&d->net());  // odd chunks of a mixed-size batch run here
    if (w->cls) v.push_back(&w->cls->net());
    v.push_back(&w->rec.net());
  }
  return v;
}
static std::vector<std::pair<const char*, SrvNet*>> pipe_srv_nets(ocr_pipe* h) {  // the server networks of a configs[4] pipeline
  std::vector<std::pair<const char*, SrvNet*>> v;
  for (PipeWorker* w : h->workers()) {
    if (w->det.srv()) v.push_back({"det.", w->det.srv()});
    if (w->rec.srv()) v.push_back({"rec.", w->rec.srv()});
  }
  return v;
}
int ocr_pipe_timing(ocr_pipe* h, int enable) {
  if (!h) return fail(OCR_ERR_ARG, "null handle");
  for (Net* net : pipe_nets(h)) {
    net->enable_timing(enable != 0);
    net->reset_timings();
  }
  for (auto& net : pipe_srv_nets(h)) {
    net.second->enable_timing(enable != 0);
    net.second->reset_timings();
  }
  for (PipeWorker* w : h->workers()) w->timing_on = enable != 0;
  return OCR_OK;
}
int ocr_pipe_stats(ocr_pipe* h, long long out[3]) {
  if (!h || !out) return fail(OCR_ERR_ARG, "null argument");
  out[0] = out[1] = out[2] = 0;
  for (Net* n : pipe_nets(h)) { out[0] += n->stats().runs; out[1] += n->stats().binds; out[2] += n->stats().graph_replays; }
  return OCR_OK;
}
int ocr_pipe_timing_filter(ocr_pipe* h, const char* substr) {
  if (!h) return fail(OCR_ERR_ARG, "null handle");
  const std::string f = substr ? substr : "";
  for (Net* net : pipe_nets(h)) net->set_timing_filter(f);
  for (PipeWorker* w : h->workers()) w->timing_filter = f;
  return OCR_OK;
}
int ocr_pipe_timing_report(ocr_pipe* h, char* buf, size_t cap) {
  if (!h || !buf) return fail(OCR_ERR_ARG, "null argument");
  size_t off = 0;
  // the halves of a split rec launch (and equal shapes on different lanes) have the same instance names: one row per name
  std::map<std::string, KernelTiming> all;
  auto add = [&](const std::string& name, const auto& k) {
    KernelTiming& t = all[name];
    t.ms += k.ms; t.count += k.count; t.flops += k.flops; t.bytes += k.bytes;
  };
  for (Net* net : pipe_nets(h))
    for (auto& kv : net->timings()) add(kv.first, kv.second);
  for (auto& net : pipe_srv_nets(h))  // (the mobile networks' names start with "det." / "rec.": the same convention)
    for (auto& kv : net.second->timings()) add(net.first + kv.first, kv.second);
  for (auto& kv : all) {
    int n = snprintf(buf + off, cap > off ? cap - off : 0, "%s %.6f %ld %.0f %.0f\n", kv.first.c_str(), kv.second.ms,
                     kv.second.count, kv.second.flops, kv.second.bytes);
    if (n < 0 || off + n >= cap) return fail(OCR_ERR_CAPACITY, "report buffer too small");
    off += n;
  }
  if (off < cap) buf[off] = 0;
  return OCR_OK;
}

int ocr_rotate_crop_shape(int rows, int cols, const int32_t* box, int* out_rows, int* out_cols) {
  if (!box || !out_rows || !out_cols) return fail(OCR_ERR_ARG, "null argument");
  CropPlan p;
  if (!plan_rotate_crop(rows, cols, box, p)) return fail(OCR_ERR_ARG, "box has no crop inside the image");
  *out_rows = p.orows;
  *out_cols = p.ocols;
  return OCR_OK;
}

int ocr_rotate_crop(const uint8_t* bgr, int rows, int cols, size_t row_stride, const int32_t* boxes, int n, uint8_t* out,
                    size_t out_cap, size_t* out_off, int* out_rows, int* out_cols) {
  if (!bgr || rows <= 0 || cols <= 0 || !boxes || n < 1 || !out || !out_off || !out_rows || !out_cols)
    return fail(OCR_ERR_ARG, "bad argument");
  const size_t row = (size_t)cols * 3, stride = row_stride ? row_stride : row;
  std::vector<WarpDesc> wd(n);
  std::vector<size_t> src_off(n);
  size_t total = 0;
  int max_px = 0;
  for (int k = 0; k < n; ++k) {
    CropPlan p;
    if (!plan_rotate_crop(rows, cols, boxes + 8 * k, p)) return fail(OCR_ERR_ARG, "box has no crop inside the image");
    WarpDesc& d = wd[k];
    d.sstride = row; d.sw = p.sw; d.sh = p.sh; d.dw = p.dw; d.dh = p.dh; d.rot = p.rot; d.bw0 = p.bw0;
    src_off[k] = (size_t)p.top * row + (size_t)p.left * 3;
    memcpy(d.m, p.minv, sizeof(d.m));
    out_off[k] = total;
    out_rows[k] = p.orows;
    out_cols[k] = p.ocols;
    total += (size_t)p.dw * p.dh * 3;
    max_px = std::max(max_px, p.dw * p.dh);
  }
  out_off[n] = total;
  if (total > out_cap) return fail(OCR_ERR_CAPACITY, "crop buffer too small");
  std::string err;
  DevBuf<uint8_t> dimg, dout;
  DevBuf<WarpDesc> ddesc;
  if (!dimg.ensure(row * rows, err) || !dout.ensure(total, err) || !ddesc.ensure(n, err)) return fail(OCR_ERR_DEVICE, err);
  for (int k = 0; k < n; ++k) {
    wd[k].src = dimg.p + src_off[k];
    wd[k].dst = dout.p + out_off[k];
  }
  CAPI_HIP(g_memcpy2d(dimg.p, row, bgr, stride, row, rows, hipMemcpyHostToDevice));
  CAPI_HIP(g_memcpy(ddesc.p, wd.data(), n * sizeof(WarpDesc), hipMemcpyHostToDevice));
  launch_warp_crops(ddesc.p, n, max_px, 0);
  CAPI_HIP(hipGetLastError());
  CAPI_HIP(g_memcpy(out, dout.p, total, hipMemcpyDeviceToHost));
  return OCR_OK;
}

int ocr_rotate180_rois(uint8_t* bgr, int rows, int cols, size_t row_stride, const int32_t* rects, int n) {
  if (!bgr || rows <= 0 || cols <= 0 || !rects || n < 1) return fail(OCR_ERR_ARG, "bad argument");
  const size_t row = (size_t)cols * 3, stride = row_stride ? row_stride : row;
  std::string err;
  DevBuf<uint8_t> dimg;
  DevBuf<RotDesc> ddesc;
  DevBuf<int> dseg;
  if (!dimg.ensure(row * rows, err)) return fail(OCR_ERR_DEVICE, err);
  std::vector<RotDesc> rd(n);
  for (int k = 0; k < n; ++k) {
    const int32_t* r = rects + 4 * k;
    if (r[0] < 0 || r[1] < 0 || r[2] < 1 || r[3] < 1 || r[0] + r[2] > cols || r[1] + r[3] > rows) return fail(OCR_ERR_ARG, "rectangle outside the image");
    rd[k] = RotDesc{dimg.p, row, r[0], r[1], r[2], r[3]};
  }
  CAPI_HIP(g_memcpy2d(dimg.p, row, bgr, stride, row, rows, hipMemcpyHostToDevice));
  const int rc = rotate180_in_order(rd, ddesc, dseg, 0, err);
  if (rc) return fail(rc, err);
  CAPI_HIP(g_memcpy2d(bgr, stride, dimg.p, row, row, rows, hipMemcpyDeviceToHost));
  return OCR_OK;
}

int ocr_dev_alloc(void** p, size_t bytes) {
  if (!p) return fail(OCR_ERR_ARG, "null argument");
  CAPI_HIP(g_malloc(p, bytes));
  return OCR_OK;
}
int ocr_dev_free(void* p) { CAPI_HIP(g_free(p)); return OCR_OK; }
int ocr_dev_upload(void* dst, const void* src, size_t bytes) { CAPI_HIP(g_memcpy(dst, src, bytes, hipMemcpyHostToDevice)); return OCR_OK; }
int ocr_dev_download(void* dst, const void* src, size_t bytes) { CAPI_HIP(g_memcpy(dst, src, bytes, hipMemcpyDeviceToHost)); return OCR_OK; }
int ocr_dev_sync(void) { CAPI_HIP(hipDeviceSynchronize()); return OCR_OK; }

}  // extern "C"
