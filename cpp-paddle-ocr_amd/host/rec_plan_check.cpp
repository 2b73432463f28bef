// rec_plan_check: the recognizer's batching plan of csrc/rec_plan.h (the reference's batches and widths, the cut into
// launches) in one plain host process that links nothing of the library and nothing of HIP - what the tests run, also
// built with -fsanitize=address,undefined.  It calls the functions RecStage::run_lines calls.
// rec_plan_check <cases>: a text file of whitespace-separated integers, per case
//     imgH imgW batch_num sort_mode server max_lines_per_launch  nseg seg[0] .. seg[nseg]  w h  w h ...  (seg[nseg] lines)
//   Prints per case "case <k>" and then either "refused <code> <message>" or "items <n>", n lines "<line> <resize_w>
//   <tensor_w>", "slots <m>", m lines "<first> <count> <ragged>".  Exit status 2 for a malformed file.
// rec_plan_check --ragged-bound: the smallest tensor width whose line the ragged attention kernel does not take
//   (rec_plan::ragged_takes, which is attn_ragged_fits of its token count, says no).
#include <cstdio>
#include <string>
#include <vector>

#include "../csrc/rec_plan.h"

using namespace ocr;

struct LineSize { int w, h; };

static bool read_ints(FILE* f, int* out, int n) {
  for (int i = 0; i < n; ++i)
    if (fscanf(f, "%d", out + i) != 1) return false;
  return true;
}

int main(int argc, char** argv) {
  const std::string mode = argc > 1 ? argv[1] : "";
  if (mode == "--ragged-bound" && argc == 2) {
    int w = 8;
    while (w < (1 << 20) && rec_plan::ragged_takes(w)) ++w;
    printf("%d\n", w);
    return 0;
  }
  if (argc != 2 || mode.empty() || mode[0] == '-') {
    fprintf(stderr, "usage: rec_plan_check <cases> | --ragged-bound\n");
    return 2;
  }
  FILE* f = fopen(argv[1], "r");
  if (!f) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
  int head[7];
  for (int k = 0; read_ints(f, head, 7); ++k) {
    const int imgH = head[0], imgW = head[1], batch_num = head[2], sort_mode = head[3], server = head[4], max_lines = head[5], nseg = head[6];
    if (imgH < 1 || imgW < 1 || batch_num < 1 || max_lines < 1 || nseg < 0 || nseg > (1 << 16)) return 2;
    std::vector<int> seg(nseg + 1);
    if (!read_ints(f, seg.data(), nseg + 1) || seg[0] != 0) return 2;
    for (int s = 0; s < nseg; ++s)
      if (seg[s + 1] < seg[s]) return 2;
    if (seg[nseg] > (1 << 20)) return 2;
    std::vector<LineSize> lines(seg[nseg]);
    for (LineSize& l : lines)
      if (!read_ints(f, &l.w, 1) || !read_ints(f, &l.h, 1) || l.w < 1 || l.h < 1) return 2;
    printf("case %d\n", k);
    std::vector<rec_plan::Item> items;
    std::string err;
    if (const int rc = rec_plan::plan_items(lines, seg, imgH, imgW, batch_num, sort_mode, server != 0, items, err)) {
      printf("refused %d %s\n", rc, err.c_str());
      continue;
    }
    printf("items %zu\n", items.size());
    for (const rec_plan::Item& it : items) printf("%d %d %d\n", it.line, it.resize_w, it.tensor_w);
    const std::vector<rec_plan::Slot> slots = rec_plan::plan_slots(items, imgH, imgW, max_lines, server != 0);
    printf("slots %zu\n", slots.size());
    for (const rec_plan::Slot& s : slots) printf("%d %d %d\n", s.first, s.count, (int)s.ragged);
  }
  const bool whole = feof(f);
  fclose(f);
  return whole ? 0 : 2;
}
