// tiff_plan_check: the plan of a coded TIFF batch of csrc/tiff_plan.h (frame offsets and padding, the chunk records in the
// order of the launch, the image descriptors of the pixel stage, the Deflate verdict) in one plain host process that links
// nothing of the library and nothing of HIP - what the tests run, also built with -fsanitize=address,undefined.  It calls the
// functions capi_tiff.hip calls.  No chunk byte is looked at: the frames carry records and a pool length, and no pool.
// tiff_plan_check < cases: whitespace-separated tokens on standard input, per case one of
//     batch <route: 0 coded | 1 deflate | 2 fax> <count> frame ...
//       frame: <width> <height> <photometric> <bits> <samples> <planar> <predictor> <tile_width> <tile_height> <compression>
//              <t4_options> <bytes_len> <nchunks>  byte_off byte_len rows ...
//       a deflate batch goes on: <verdicts>, per verdict <with ids: 0 | 1> [id per frame] and `produced` per chunk in batch order
//     bound <nchunks>
//   Prints "case <k>" and then, for a batch: "frames <n>", n lines "<off> <pool_at> <first_chunk> <total> <chunk_bytes>
//   <row_bytes>", "sizes <bytes> <pool> <nchunks> <record_bytes> <at_pool> <coded_bytes> <lzw> <runs>", "records <m>", m lines
//   "<frame> <chunk> <src> <dst> <byte_len>" and then coded: "<need> <nominal> <compression>", deflate: "<need> <nominal>", fax:
//   "<rows> <nominal> <width> <compression> <t4_options>"; "kinds" and per kind "<first> <count> <units>" on one line; "descs <n>",
//   n lines "<data - base> <first_unit> <chunk_bytes> <plane_bytes> <row_bytes> <width> <height> <tile_width> <tile_height>
//   <across> <down> <bits> <samples> <used> <mode> <predictor> <big_endian> <invert> <premultiply> <lanes_per_row> <rows_per_unit>
//   <units_per_chunk>"; per verdict "short <record, or -1>" and, where a chunk fell short, a line with the refusal's text.
//   A frame that tiff_fault refuses: "refused <i> <text>" ends the case.  For a bound: "fits <0 | 1>".
//   Exit status 2 for malformed input.
#include <cstdio>
#include <string>
#include <vector>

#include "../csrc/tiff_plan.h"

using namespace ocr;
namespace tiff = PaddleOCR::tiff;

static bool read_ints(long long* out, int n) {
  for (int i = 0; i < n; ++i)
    if (scanf("%lld", out + i) != 1) return false;
  return true;
}
static bool in_range(long long v, long long lo, long long hi) { return v >= lo && v <= hi; }

static bool batch_case() {
  long long head[2];
  if (!read_ints(head, 2) || !in_range(head[0], 0, 2) || !in_range(head[1], 0, 64)) return false;
  const tiff_plan::Route route = (tiff_plan::Route)head[0];
  const int count = (int)head[1];
  std::vector<ocr_tiff_fax> frames((size_t)count);  // (every route: a coded frame is the first member of one)
  std::vector<std::vector<ocr_tiff_chunk>> chunks((size_t)count);
  for (int i = 0; i < count; ++i) {
    long long v[13];
    if (!read_ints(v, 13) || !in_range(v[11], 0, 1 << 20) || !in_range(v[12], 0, 1 << 12)) return false;
    for (int k = 0; k < 11; ++k)
      if (!in_range(v[k], -(1 << 20), 1 << 20)) return false;
    frames[i] = ocr_tiff_fax();
    ocr_tiff_coded& c = frames[i].coded;
    ocr_tiff_frame& f = c.frame;
    f.width = (int)v[0]; f.height = (int)v[1]; f.photometric = (int)v[2]; f.bits_per_sample = (int)v[3]; f.samples_per_pixel = (int)v[4];
    f.planar = (int)v[5]; f.predictor = (int)v[6]; f.tile_width = (int)v[7]; f.tile_height = (int)v[8];
    c.compression = (int)v[9];
    frames[i].t4_options = (uint32_t)v[10];
    c.bytes_len = (size_t)v[11];
    chunks[i].resize((size_t)v[12]);
    for (ocr_tiff_chunk& ch : chunks[i]) {
      long long r[3];
      if (!read_ints(r, 3) || !in_range(r[0], 0, 1 << 20) || !in_range(r[1], 0, 1 << 20) || !in_range(r[2], 0, 1 << 20)) return false;
      ch = ocr_tiff_chunk{(uint64_t)r[0], (uint32_t)r[1], (uint32_t)r[2]};
    }
    c.chunks = chunks[i].data();
    c.chunks_len = chunks[i].size();
  }
  std::vector<const ocr_tiff_coded*> imgs((size_t)count);
  tiff_plan::Plan P;
  P.route = route;
  P.geo.resize((size_t)count);
  for (int i = 0; i < count; ++i) {
    imgs[i] = &frames[i].coded;
    if (const char* why = tiff_plan::tiff_fault(imgs[i]->frame, P.geo[i], false)) { printf("refused %d %s\n", i, why); return true; }
    if (imgs[i]->chunks_len != (size_t)P.geo[i].across * P.geo[i].down * P.geo[i].planes) return false;  // (the rule of the records)
  }
  if (!tiff_plan::build(P, imgs.data(), count)) return false;
  printf("frames %d\n", count);
  for (int i = 0; i < count; ++i)
    printf("%zu %zu %zu %zu %zu %zu\n", P.off[i], P.pool_at[i], P.first_chunk[i], P.geo[i].total, P.geo[i].chunk_bytes, P.geo[i].row_bytes);
  printf("sizes %zu %zu %zu %zu %zu %zu %u %u\n", P.bytes, P.pool, P.nchunks, P.record_bytes, P.at_pool, P.coded_bytes, P.lzw, P.runs);
  printf("records %zu\n", P.whose.size());
  for (size_t n = 0; n < P.whose.size(); ++n) {
    printf("%d %u ", P.whose[n].frame, P.whose[n].chunk);
    if (route == tiff_plan::kCoded) {
      const TiffChunkDesc& r = ((const TiffChunkDesc*)P.records())[n];
      printf("%llu %llu %u %u %u %u\n", (unsigned long long)r.src, (unsigned long long)r.dst, r.byte_len, r.need, r.nominal, r.compression);
    } else if (route == tiff_plan::kDeflate) {
      const InflateDesc& r = ((const InflateDesc*)P.records())[n];
      printf("%llu %llu %u %u %u\n", (unsigned long long)r.src, (unsigned long long)r.dst, r.byte_len, r.need, r.nominal);
    } else {
      const TiffFaxDesc& r = ((const TiffFaxDesc*)P.records())[n];
      printf("%llu %llu %u %u %u %u %u %u\n", (unsigned long long)r.src, (unsigned long long)r.dst, r.byte_len, r.rows, r.nominal, r.width, r.compression, r.t4_options);
    }
  }
  tiff_plan::Kinds K;
  const std::vector<uint8_t> base(P.bytes + 1);  // stands for the device buffer of the expanded chunks: only addresses are taken
  const std::vector<TiffImageDesc> id = tiff_plan::describe(imgs.data(), count, P.geo, P.off, nullptr, base.data(), K);
  printf("kinds");
  for (int k = 0; k < kTiffKinds; ++k) printf(" %d %d %llu", K.first[k], K.count[k], K.units[k]);
  printf("\ndescs %zu\n", id.size());
  for (const TiffImageDesc& d : id)
    printf("%zu %llu %zu %zu %zu %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %u\n", (size_t)(d.data - base.data()), d.first_unit, d.chunk_bytes, d.plane_bytes,
           d.row_bytes, d.width, d.height, d.tile_width, d.tile_height, d.across, d.down, d.bits, d.samples, d.used, d.mode, d.predictor, d.big_endian, d.invert,
           d.premultiply, d.lanes_per_row, d.rows_per_unit, d.units_per_chunk);
  if (route != tiff_plan::kDeflate) return true;
  long long verdicts;
  if (!read_ints(&verdicts, 1) || !in_range(verdicts, 0, 16)) return false;
  for (long long v = 0; v < verdicts; ++v) {
    long long with_ids;
    if (!read_ints(&with_ids, 1) || !in_range(with_ids, 0, 1)) return false;
    std::vector<int> ids;
    for (int i = 0; i < count && with_ids; ++i) {
      long long x;
      if (!read_ints(&x, 1) || !in_range(x, 0, 1 << 20)) return false;
      ids.push_back((int)x);
    }
    std::vector<uint32_t> batch_order(P.nchunks), produced(P.whose.size());
    for (uint32_t& x : batch_order) {
      long long y;
      if (!read_ints(&y, 1) || !in_range(y, 0, 1 << 20)) return false;
      x = (uint32_t)y;
    }
    for (size_t n = 0; n < P.whose.size(); ++n) produced[n] = batch_order[P.first_chunk[P.whose[n].frame] + P.whose[n].chunk];  // as the launch reports them
    const size_t bad = tiff_plan::first_short(P, produced.data());
    printf("short %lld\n", bad < P.whose.size() ? (long long)bad : -1LL);
    if (bad < P.whose.size()) printf("%s\n", tiff_plan::short_text(P, bad, with_ids ? ids.data() : nullptr).c_str());
  }
  return true;
}

static bool bound_case() {
  long long n;
  if (!read_ints(&n, 1) || n < 0) return false;
  printf("fits %d\n", (int)tiff_plan::chunks_fit_a_launch((size_t)n));
  return true;
}

int main() {
  char kind[16];
  for (int k = 0; scanf("%15s", kind) == 1; ++k) {
    printf("case %d\n", k);
    const std::string s = kind;
    if (!(s == "batch" ? batch_case() : s == "bound" && bound_case())) return 2;
  }
  return feof(stdin) ? 0 : 2;
}
