// The recognizer's batching plan: which lines share a batch of the reference, what width each line is resized and padded
// to, and how the lines of a call are cut into launches.  Host arithmetic only - no HIP, no device types - so that a plain
// host program (host/rec_plan_check.cpp) runs exactly what RecStage::run_lines runs.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <string>
#include <vector>

#include "../../include/ocr_hip.h"

namespace ocr {

// LDS working set of the ragged-capable attention kernel (kernels_net.hip, attn_lds_kernel) for sequences of T tokens
inline size_t attn_lds_bytes(int T) { return ((size_t)T * 96 + 64 * 17) * sizeof(float); }
// does the ragged form of the attention kernel take sequences of this length? (its working set must fit LDS)
inline bool attn_ragged_fits(int T) { return attn_lds_bytes(T) <= 150 * 1024; }

namespace rec_plan {

struct Item { int line, resize_w, tensor_w; };  // a line of the call: its index, the width it is resized to, its tensor's width
struct Slot { int first, count; bool ragged; };  // one launch: items [first, first + count)

// CrnnResizeImg / ClsResizeImg: the resized width of a w x h line in a tensor of height imgH, at most `limit`
inline int rec_resize_w(int w, int h, int imgH, int limit) {
  const float ratio = float(w) / float(h);
  return ceilf(imgH * ratio) > limit ? limit : int(ceilf(imgH * ratio));
}

// CTC steps a uniform launch of this tensor width can leave per line, at most (what the step buffers are sized by)
inline int uniform_step_cap(int tensor_w) { return tensor_w / 4 + 8; }

// CRNNRecognizer::Run batching, src/ocr_rec.cpp:34-57, inside each segment seg[s] .. seg[s + 1] of `lines` (one image's
// lines; Line has int w, h): the items of all segments, stable-sorted by tensor width.  The float / double mix of the
// expressions is the reference's.  fixed_width: the server recognizer's one token grid (every tensor is imgW wide).
// Returns OCR_OK, or OCR_ERR_ARG with `err` set where OCR_SORT_MSVC_STRICT refuses.
template <class Line>
inline int plan_items(const std::vector<Line>& lines, const std::vector<int>& seg, int imgH, int imgW, int batch_num, int sort_mode,
                      bool fixed_width, std::vector<Item>& items, std::string& err) {
  items.clear();
  items.reserve(lines.size());
  for (size_t sg = 0; sg + 1 < seg.size(); ++sg) {
    const int s0 = seg[sg], sn = seg[sg + 1] - seg[sg];
    std::vector<float> width_list(sn);
    for (int i = 0; i < sn; ++i) width_list[i] = float(lines[s0 + i].w) / lines[s0 + i].h;
    std::vector<size_t> indices(sn);
    for (int i = 0; i < sn; ++i) indices[i] = i;
    // Utility::argsort is std::sort: the order of equal ratios is the host library's
    if (sort_mode == OCR_SORT_MSVC_STRICT && sn > 32) {
      // MSVC's std::sort is an insertion sort (ties in input order) only up to _ISORT_MAX = 32 elements; its quicksort's order
      // of ties beyond that is not restated here - refuse rather than answer in an order the reference's build may not produce
      std::vector<float> sorted_w(width_list);
      std::sort(sorted_w.begin(), sorted_w.end());
      if (std::adjacent_find(sorted_w.begin(), sorted_w.end()) != sorted_w.end()) {
        char msg[200];
        snprintf(msg, sizeof msg, "sort_mode OCR_SORT_MSVC_STRICT: image %d has %d crops (> 32) with tied w/h ratios - MSVC's std::sort order of ties beyond 32 elements is not restated (use OCR_SORT_STABLE or OCR_SORT_STD)", (int)sg, sn);
        err = msg;
        return OCR_ERR_ARG;
      }
    }
    if (sort_mode != OCR_SORT_STD) std::stable_sort(indices.begin(), indices.end(), [&](size_t a, size_t b) { return width_list[a] < width_list[b]; });
    else std::sort(indices.begin(), indices.end(), [&](size_t a, size_t b) { return width_list[a] < width_list[b]; });
    for (int beg = 0; beg < sn; beg += batch_num) {
      const int end = std::min(sn, beg + batch_num);
      float max_wh_ratio = imgW * 1.0 / imgH;
      for (int ino = beg; ino < end; ++ino) {
        const int h = lines[s0 + indices[ino]].h, w = lines[s0 + indices[ino]].w;
        const float wh_ratio = w * 1.0 / h;
        max_wh_ratio = std::max(max_wh_ratio, wh_ratio);
      }
      if (fixed_width) max_wh_ratio = imgW * 1.0 / imgH;
      const int bw = int(imgH * max_wh_ratio);  // CrnnResizeImg: imgW = int(imgH * wh_ratio)
      const int tensor_w = std::max(bw, imgW);
      for (int ino = beg; ino < end; ++ino) {
        const Line& L = lines[s0 + indices[ino]];
        items.push_back({s0 + (int)indices[ino], rec_resize_w(L.w, L.h, imgH, bw), tensor_w});
      }
    }
  }
  std::stable_sort(items.begin(), items.end(), [](const Item& a, const Item& b) { return a.tensor_w < b.tensor_w; });
  return OCR_OK;
}

// does a ragged launch take a line of this tensor width? (its attention sequence: a token per 8 columns and 2)
inline bool ragged_takes(int tensor_w) { return attn_ragged_fits(tensor_w / 8 + 2); }

// pixels of activation one launch may hold: max_lines_per_launch lines of 48 x 320 (or of the configured shape, if wider)
inline long launch_budget(int imgH, int imgW, int max_lines_per_launch) { return (long)max_lines_per_launch * imgH * std::max(imgW, 320); }

// One launch list for every tensor width of the call (a ragged batch: kernels_net.h, RagLevel).  In the reference each
// batch of rec_batch_num lines is a predictor run of its own width (ocr_rec.cpp:47-81); a line's results depend on
// its own tensor width only (padding, attention length), never on the other lines of a launch, so the lines of all
// batches - and of all images of a request batch - share the launches.  Lines in ascending tensor width (equal
// widths stay neighbours: a workgroup's tiles then belong to lines of one shape); a launch is cut where its
// activation arena would pass the pixel budget; a line too wide for the ragged attention kernel's LDS working set
// (> ~3000 px) runs as a uniform launch of its own width, and so does every line with uniform_only (the server net).
inline std::vector<Slot> plan_slots(const std::vector<Item>& items, int imgH, int imgW, int max_lines_per_launch, bool uniform_only) {
  std::vector<Slot> slots;
  const long budget = launch_budget(imgH, imgW, max_lines_per_launch);
  const auto fits = [&](int i) { return ragged_takes(items[i].tensor_w); };
  int i = 0;
  const int ni = (int)items.size();
  while (i < ni) {
    if (uniform_only || !fits(i)) {  // uniform launch: the lines of exactly this width
      int j = i;
      while (j < ni && items[j].tensor_w == items[i].tensor_w && j - i < max_lines_per_launch) ++j;
      slots.push_back({i, j - i, false});
      i = j;
      continue;
    }
    long pix = 0;
    int j = i;
    while (j < ni && fits(j) && (j == i || pix + (long)imgH * items[j].tensor_w <= budget)) {
      pix += (long)imgH * items[j].tensor_w;
      ++j;
    }
    slots.push_back({i, j - i, true});
    i = j;
  }
  return slots;
}

}  // namespace rec_plan
}  // namespace ocr
