// The pipeline's batch plan: the detector's resize shape, a slot's layout (image order, size groups, byte and probability
// offsets), the split of a batch over the chains, the detector's chunks, the bounding-rectangle crops and the hand-over of
// the results.  Host arithmetic only - no HIP, no device types - so that a plain host program (host/pipe_plan_check.cpp)
// runs exactly what pipe.hip runs.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "../../include/ocr_hip.h"

namespace ocr {
namespace pipe_plan {

// ResizeImgType0::Run, preprocess_op.cpp:57-93: the detector's input shape for an h x w image
inline void det_resize_shape(int h, int w, const std::string& limit_type, int limit_side_len, int& rh, int& rw, float& ratio_h,
                             float& ratio_w) {
  float ratio = 1.f;
  if (limit_type == "min") {
    const int min_wh = std::min(h, w);
    if (min_wh < limit_side_len) ratio = h < w ? float(limit_side_len) / float(h) : float(limit_side_len) / float(w);
  } else {
    const int max_wh = std::max(h, w);
    if (max_wh > limit_side_len) ratio = h > w ? float(limit_side_len) / float(h) : float(limit_side_len) / float(w);
  }
  const int resize_h = int(float(h) * ratio), resize_w = int(float(w) * ratio);
  rh = std::max(int(std::round(float(resize_h) / 32) * 32), 32);
  rw = std::max(int(std::round(float(resize_w) / 32) * 32), 32);
  ratio_h = float(rh) / float(h);
  ratio_w = float(rw) / float(w);
}
// pixels of that shape: the floats of an image's probability map
inline size_t det_pixels(int h, int w, const std::string& limit_type, int limit_side_len) {
  int rh = 0, rw = 0;
  { float a, b; det_resize_shape(h, w, limit_type, limit_side_len, rh, rw, a, b); }
  return (size_t)rh * rw;
}

struct Img { int rows, cols, orig; size_t off, prob_off; };                // orig: the image's place in the caller's batch
struct Group { int rows, cols, first, count; size_t off, prob_off; };      // images [first, first + count) of the layout
struct Layout { std::vector<Img> imgs; std::vector<Group> groups; size_t bytes = 0, prob_floats = 0; };  // imgs in layout order

// layout of a batch in a slot: stable order by (rows, cols), images of one size contiguous (one size group: one det pass),
// every group on a 256-byte boundary; probability maps (benchmark protocol) packed in the same order
inline Layout layout(const std::vector<std::pair<int, int>>& sizes /* rows, cols */, const std::string& limit_type, int limit_side_len) {
  const int count = (int)sizes.size();
  std::vector<int> order(count);
  for (int i = 0; i < count; ++i) order[i] = i;
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return sizes[a] < sizes[b]; });
  Layout L;
  size_t off = 0, poff = 0;
  for (int k = 0; k < count; ++k) {
    const int r = sizes[order[k]].first, c = sizes[order[k]].second;
    if (L.groups.empty() || L.groups.back().rows != r || L.groups.back().cols != c) {
      off = (off + 255) & ~(size_t)255;
      L.groups.push_back({r, c, k, 0, off, poff});
    }
    L.groups.back().count++;
    L.imgs.push_back({r, c, order[k], off, poff});
    off += (size_t)r * c * 3;
    poff += det_pixels(r, c, limit_type, limit_side_len);
  }
  L.bytes = off; L.prob_floats = poff;
  return L;
}

// probability maps attached to a slot stay valid only while the layout is the same
inline bool same_layout(const std::vector<Img>& before, const std::vector<Img>& after) {
  bool same = before.size() == after.size();
  for (size_t k = 0; same && k < before.size(); ++k)
    same = before[k].rows == after[k].rows && before[k].cols == after[k].cols && before[k].orig == after[k].orig;
  return same;
}

// a chain's part of a batch: its groups' first / off / prob_off are re-based to the part; index: the layout index of its images
struct Part { std::vector<Img> imgs; std::vector<Group> groups; std::vector<int> index; };

// K parts of a batch, one per chain: size groups dealt to the lightest part (pixels), a group cut where that part reaches its
// share of the batch
inline std::vector<Part> split(const std::vector<Img>& imgs, const std::vector<Group>& groups, int K, const std::string& limit_type,
                               int limit_side_len) {
  std::vector<Part> parts(K);
  std::vector<size_t> load(K, 0);
  size_t total = 0;
  for (const auto& g : groups) total += (size_t)g.count * g.rows * g.cols;
  const size_t share = (total + K - 1) / K;
  for (const auto& g : groups) {
    const size_t px = (size_t)g.rows * g.cols, ppx = det_pixels(g.rows, g.cols, limit_type, limit_side_len);
    int first = 0;
    while (first < g.count) {
      const int p = (int)(std::min_element(load.begin(), load.end()) - load.begin());
      const int left = g.count - first;
      const size_t room = share > load[p] ? share - load[p] : 0;
      int n = left;
      if ((size_t)left * px > room + px / 2) n = (int)std::min<size_t>(left, std::max<size_t>(1, (room + px / 2) / px));
      Group ng = g;  // images first .. first + n - 1 of group g
      ng.first = (int)parts[p].imgs.size();
      ng.count = n;
      ng.off = g.off + (size_t)first * px * 3;
      ng.prob_off = g.prob_off + (size_t)first * ppx;
      parts[p].groups.push_back(ng);
      for (int k = 0; k < n; ++k) { parts[p].imgs.push_back(imgs[g.first + first + k]); parts[p].index.push_back(g.first + first + k); }
      load[p] += (size_t)n * px;
      first += n;
    }
  }
  return parts;
}

// the chunks [g0, g1) of a ragged detector pass: a chunk always takes its first group, and further groups while the sum of
// their detector-input pixels stays within the budget (what bounds the activation arena)
inline std::vector<std::pair<size_t, size_t>> det_chunks(const std::vector<size_t>& group_pixels, size_t budget) {
  std::vector<std::pair<size_t, size_t>> chunks;
  for (size_t g0 = 0; g0 < group_pixels.size();) {
    size_t g1 = g0, px = 0;
    while (g1 < group_pixels.size() && (g1 == g0 || px + group_pixels[g1] <= budget)) px += group_pixels[g1++];
    chunks.emplace_back(g0, g1);
    g0 = g1;
  }
  return chunks;
}

// crop rectangle of a box (4 points): cv::boundingRect(points) & image rect (ocr_worker.cpp:245-258); false: empty, no crop
inline bool rect_crop(const int32_t* b, int rows, int cols, int& x, int& y, int& w, int& h) {
  int x0 = b[0], x1 = b[0], y0 = b[1], y1 = b[1];
  for (int k = 1; k < 4; ++k) {
    x0 = std::min(x0, b[2 * k]); x1 = std::max(x1, b[2 * k]);
    y0 = std::min(y0, b[2 * k + 1]); y1 = std::max(y1, b[2 * k + 1]);
  }
  x = std::max(x0, 0); y = std::max(y0, 0);
  w = std::min(x1 + 1, cols) - x; h = std::min(y1 + 1, rows) - y;
  return w > 0 && h > 0;
}

struct RectLine { int x, y, w, h, box; };  // a text line of an image: its crop, and the box its word reports
// the lines of one image's nbox boxes.  `word.box = det_boxes[i]` pairs text k with box k of the image, even when an empty
// crop was skipped before it (reference quirk, ocr_worker.cpp:293-299) - kept: `box` is the line's running index.
inline void rect_lines(const int32_t* boxes, int nbox, int rows, int cols, std::vector<RectLine>& out) {
  out.clear();
  for (int j = 0; j < nbox; ++j) {
    RectLine l{0, 0, 0, 0, (int)out.size()};
    if (rect_crop(boxes + (size_t)j * 8, rows, cols, l.x, l.y, l.w, l.h)) out.push_back(l);
  }
}

using CharLists = std::vector<std::vector<ocr_char>>;  // per image: one ocr_char per class id (ocr_pipe_run_chars)
// The results of a batch into the caller's arrays, image i of the caller from entry order[i] of W / I / C.  false: the
// result buffers are too small (word_off / nwords are written up to and including the image that did not fit).
inline bool emit(const std::vector<std::vector<ocr_word>>& W, const std::vector<std::vector<int32_t>>& I, const std::vector<int>& order,
                 ocr_word* words, int cap_words, int* word_off, int* nwords, int32_t* ids, int cap_ids, const CharLists* C = nullptr,
                 ocr_char* chars = nullptr) {
  int wo = 0, io = 0;
  for (size_t i = 0; i < order.size(); ++i) {
    const auto& w = W[order[i]];
    const auto& d = I[order[i]];
    word_off[i] = wo; nwords[i] = (int)w.size();
    if (wo + (int)w.size() > cap_words || io + (int)d.size() > cap_ids) return false;
    for (size_t k = 0; k < w.size(); ++k) {
      words[wo + k] = w[k];
      words[wo + k].ids_off += io;
    }
    if (!d.empty()) memcpy(ids + io, d.data(), d.size() * sizeof(int32_t));
    if (C && chars && !d.empty()) memcpy(chars + io, (*C)[order[i]].data(), d.size() * sizeof(ocr_char));
    wo += (int)w.size(); io += (int)d.size();
  }
  return true;
}

}  // namespace pipe_plan
}  // namespace ocr
