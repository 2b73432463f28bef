// pipe_plan_check: the pipeline's batch plan of csrc/pipe_plan.h (resize shape, slot layout, split over the chains, detector
// chunks, bounding-rectangle crops) in one plain host process that links nothing of the library and nothing of HIP - what the
// tests run, also built with -fsanitize=address,undefined.  It calls the functions pipe.hip calls.
// pipe_plan_check <cases>: a text file of whitespace-separated tokens, per case one of
//     batch <min: 0 | 1> <limit_side_len> <nbudgets> budget ...  <count> rows cols  rows cols ...
//     crops <rows> <cols> <nbox>  x0 y0 x1 y1 x2 y2 x3 y3 ...
//   Prints "case <k>" and then, for a batch: "imgs <n>", n lines "<rows> <cols> <orig> <off> <prob_off> <rh> <rw> <ratio_h>
//   <ratio_w>" (ratios as %a), "groups <m>", m lines "<rows> <cols> <first> <count> <off> <prob_off>", "bytes <b> probs <p>",
//   "same <this layout against itself> <against the batch case before it>"; per budget "chunks <budget> <c>" and c lines "<g0> <g1>";
//   for chains = 1 .. 4 (while the batch is not empty) "split <chains> <K>" and per part "part <images> <groups>", its image
//   lines "<layout index> <rows> <cols> <orig> <off> <prob_off>" and its group lines as above.
//   For crops: "rects <nbox>", per box "<ok> <x> <y> <w> <h>", then "lines <n>" and n lines "<x> <y> <w> <h> <box>".
//   Exit status 2 for a malformed file.
#include <cstdio>
#include <string>
#include <vector>

#include "../csrc/pipe_plan.h"

using namespace ocr;

static bool read_ints(FILE* f, long long* out, int n) {
  for (int i = 0; i < n; ++i)
    if (fscanf(f, "%lld", out + i) != 1) return false;
  return true;
}
static bool in_range(long long v, long long lo, long long hi) { return v >= lo && v <= hi; }

static void print_groups(const std::vector<pipe_plan::Group>& groups) {
  for (const auto& g : groups) printf("%d %d %d %d %zu %zu\n", g.rows, g.cols, g.first, g.count, g.off, g.prob_off);
}

static bool batch_case(FILE* f, std::vector<pipe_plan::Img>& previous) {
  long long head[3];
  if (!read_ints(f, head, 3) || !in_range(head[0], 0, 1) || !in_range(head[1], 1, 1 << 16) || !in_range(head[2], 0, 64)) return false;
  const std::string limit_type = head[0] ? "min" : "max";
  const int side = (int)head[1];
  std::vector<long long> budgets(head[2]);
  long long count;
  if (!read_ints(f, budgets.data(), (int)budgets.size()) || !read_ints(f, &count, 1) || !in_range(count, 0, 1 << 16)) return false;
  std::vector<std::pair<int, int>> sizes(count);
  for (auto& s : sizes) {
    long long rc[2];
    if (!read_ints(f, rc, 2) || !in_range(rc[0], 1, 1 << 14) || !in_range(rc[1], 1, 1 << 14)) return false;
    s = {(int)rc[0], (int)rc[1]};
  }
  const pipe_plan::Layout L = pipe_plan::layout(sizes, limit_type, side);
  printf("imgs %zu\n", L.imgs.size());
  for (const auto& im : L.imgs) {
    int rh = 0, rw = 0;
    float fh = 0, fw = 0;
    pipe_plan::det_resize_shape(im.rows, im.cols, limit_type, side, rh, rw, fh, fw);
    printf("%d %d %d %zu %zu %d %d %a %a\n", im.rows, im.cols, im.orig, im.off, im.prob_off, rh, rw, fh, fw);
  }
  printf("groups %zu\n", L.groups.size());
  print_groups(L.groups);
  printf("bytes %zu probs %zu\n", L.bytes, L.prob_floats);
  printf("same %d %d\n", (int)pipe_plan::same_layout(L.imgs, L.imgs), (int)pipe_plan::same_layout(previous, L.imgs));
  previous = L.imgs;
  std::vector<size_t> gpx;
  for (const auto& g : L.groups) gpx.push_back((size_t)g.count * pipe_plan::det_pixels(g.rows, g.cols, limit_type, side));
  for (long long b : budgets) {
    if (b < 0) return false;
    const auto chunks = pipe_plan::det_chunks(gpx, (size_t)b);
    printf("chunks %lld %zu\n", b, chunks.size());
    for (const auto& c : chunks) printf("%zu %zu\n", c.first, c.second);
  }
  for (int chains = 1; chains <= 4 && count > 0; ++chains) {
    const int K = (int)std::min<long long>(chains, count);
    const std::vector<pipe_plan::Part> parts = pipe_plan::split(L.imgs, L.groups, K, limit_type, side);
    printf("split %d %d\n", chains, K);
    for (const auto& p : parts) {
      printf("part %zu %zu\n", p.imgs.size(), p.groups.size());
      for (size_t k = 0; k < p.imgs.size(); ++k)
        printf("%d %d %d %d %zu %zu\n", p.index[k], p.imgs[k].rows, p.imgs[k].cols, p.imgs[k].orig, p.imgs[k].off, p.imgs[k].prob_off);
      print_groups(p.groups);
    }
  }
  return true;
}

static bool crops_case(FILE* f) {
  long long head[3];
  if (!read_ints(f, head, 3) || !in_range(head[0], 1, 1 << 14) || !in_range(head[1], 1, 1 << 14) || !in_range(head[2], 0, 1 << 16)) return false;
  const int rows = (int)head[0], cols = (int)head[1], nbox = (int)head[2];
  std::vector<int32_t> boxes((size_t)nbox * 8);
  for (int32_t& v : boxes) {
    long long x;
    if (!read_ints(f, &x, 1) || !in_range(x, -(1 << 20), 1 << 20)) return false;
    v = (int32_t)x;
  }
  printf("rects %d\n", nbox);
  for (int j = 0; j < nbox; ++j) {
    int x, y, w, h;
    const bool ok = pipe_plan::rect_crop(boxes.data() + (size_t)j * 8, rows, cols, x, y, w, h);
    printf("%d %d %d %d %d\n", (int)ok, x, y, w, h);
  }
  std::vector<pipe_plan::RectLine> lines;
  pipe_plan::rect_lines(boxes.data(), nbox, rows, cols, lines);
  printf("lines %zu\n", lines.size());
  for (const auto& l : lines) printf("%d %d %d %d %d\n", l.x, l.y, l.w, l.h, l.box);
  return true;
}

int main(int argc, char** argv) {
  if (argc != 2 || argv[1][0] == '-') {
    fprintf(stderr, "usage: pipe_plan_check <cases>\n");
    return 2;
  }
  FILE* f = fopen(argv[1], "r");
  if (!f) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
  char kind[16];
  std::vector<pipe_plan::Img> previous;
  for (int k = 0; fscanf(f, "%15s", kind) == 1; ++k) {
    printf("case %d\n", k);
    const std::string s = kind;
    if (!(s == "batch" ? batch_case(f, previous) : s == "crops" && crops_case(f))) { fclose(f); return 2; }
  }
  const bool whole = feof(f);
  fclose(f);
  return whole ? 0 : 2;
}
