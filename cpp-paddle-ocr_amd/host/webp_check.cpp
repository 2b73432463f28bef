// webp_check: the lossless WebP decoder of webp_decode.h (container, prefix codes, LZ77, colour cache, host pixel stage) in one
// plain host process that links nothing of the library - what the tests compile with -fsanitize=address,undefined.  Every
// file is copied to a heap block of exactly its size, so a read past its end is the sanitizer's to see.
// webp_check --decode <file> <out> [<file> <out> ...]: webp::parse + webp::pixels; out: the packed BGR image.  Prints
//   "<width> <height>" per file; the first refused file ends the run with exit status 1 and its reason on stderr.
// webp_check --pixels <descriptors> <out>: webp::pixels alone, over frame descriptors instead of files - what the device stage
//   is compared with.  descriptors: repeated [i32 width, height, ntransforms][u64 n][n coded ARGB dwords] and per transform
//   [i32 kind, bits][u64 n][n dwords], little-endian; out: the BGR images one after another (nothing for a refused frame:
//   the exit status is 1 then).
// webp_check --why <file> [...]: per file one line, "ok <width> <height> <device_ok>" or "refused: <reason>"; exit status 0.
// webp_check --frame <file> <descriptors>: webp::parse, then the frame in the form --pixels reads.
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <string>

#include "webp_decode.h"

using namespace PaddleOCR;

static bool read_exact(const std::string& path, std::unique_ptr<uint8_t[]>& buf, size_t& n) {
  FILE* f = fopen(path.c_str(), "rb");
  if (!f) return false;
  fseek(f, 0, SEEK_END);
  const long len = ftell(f);
  fseek(f, 0, SEEK_SET);
  if (len < 0) { fclose(f); return false; }
  n = (size_t)len;
  buf.reset(new uint8_t[n ? n : 1]);
  const bool ok = fread(buf.get(), 1, n, f) == n;
  fclose(f);
  return ok;
}

static bool parse_file(const std::string& path, webp::Frame& frame) {
  std::unique_ptr<uint8_t[]> buf;
  size_t n = 0;
  if (!read_exact(path, buf, n)) { fprintf(stderr, "cannot read %s\n", path.c_str()); exit(2); }
  return webp::parse(buf.get(), n, frame);
}

static bool read_dwords(FILE* f, std::vector<uint32_t>& v) {
  uint64_t n;
  if (fread(&n, 1, 8, f) != 8 || n > ((uint64_t)1 << 28)) return false;
  v.resize((size_t)n);
  return fread(v.data(), 4, (size_t)n, f) == n;
}
static void write_dwords(FILE* f, const std::vector<uint32_t>& v) {
  const uint64_t n = v.size();
  fwrite(&n, 1, 8, f);
  fwrite(v.data(), 4, v.size(), f);
}

static int pixels_of_frames(const char* in, const char* outp) {
  FILE* f = fopen(in, "rb");
  FILE* o = fopen(outp, "wb");
  if (!f || !o) return 2;
  int rc = 0;
  for (;;) {
    int32_t head[3];
    webp::Frame frame;
    const size_t got = fread(head, 1, sizeof head, f);
    if (got == 0) break;
    if (got != sizeof head || head[2] < 0 || head[2] > 16 || !read_dwords(f, frame.argb)) return 2;
    frame.width = head[0]; frame.height = head[1];
    frame.transforms.resize((size_t)head[2]);
    for (webp::Transform& t : frame.transforms) {
      int32_t kb[2];
      if (fread(kb, 1, sizeof kb, f) != sizeof kb || !read_dwords(f, t.data)) return 2;
      t.kind = kb[0]; t.bits = kb[1];
    }
    std::vector<uint8_t> bgr;
    if (!webp::pixels(frame, bgr)) { rc = 1; continue; }
    fwrite(bgr.data(), 1, bgr.size(), o);
  }
  fclose(f);
  fclose(o);
  return rc;
}

int main(int argc, char** argv) {
  const std::string mode = argc > 1 ? argv[1] : "";
  if (mode == "--pixels" && argc == 4) return pixels_of_frames(argv[2], argv[3]);
  if (mode == "--why" && argc >= 3) {
    for (int i = 2; i < argc; ++i) {
      webp::Frame frame;
      if (parse_file(argv[i], frame)) printf("ok %d %d %d\n", frame.width, frame.height, (int)frame.device_ok);
      else printf("refused: %s\n", frame.error ? frame.error : "?");
    }
    return 0;
  }
  if (mode == "--frame" && argc == 4) {
    webp::Frame frame;
    if (!parse_file(argv[2], frame)) { fprintf(stderr, "refused: %s: %s\n", argv[2], frame.error ? frame.error : "?"); return 1; }
    FILE* o = fopen(argv[3], "wb");
    if (!o) return 2;
    const int32_t head[3] = {frame.width, frame.height, (int32_t)frame.transforms.size()};
    fwrite(head, 1, sizeof head, o);
    write_dwords(o, frame.argb);
    for (const webp::Transform& t : frame.transforms) {
      const int32_t kb[2] = {t.kind, t.bits};
      fwrite(kb, 1, sizeof kb, o);
      write_dwords(o, t.data);
    }
    fclose(o);
    return 0;
  }
  if (mode == "--decode" && argc >= 4 && argc % 2 == 0) {
    for (int i = 2; i < argc; i += 2) {
      webp::Frame frame;
      std::vector<uint8_t> bgr;
      if (!parse_file(argv[i], frame) || !webp::pixels(frame, bgr)) {
        fprintf(stderr, "refused: %s: %s\n", argv[i], frame.error ? frame.error : "the frame is unsound");
        return 1;
      }
      FILE* o = fopen(argv[i + 1], "wb");
      if (!o) return 2;
      fwrite(bgr.data(), 1, bgr.size(), o);
      fclose(o);
      printf("%d %d\n", frame.width, frame.height);
    }
    return 0;
  }
  fprintf(stderr, "usage: webp_check --decode <file> <out> [...] | --pixels <descriptors> <out> | --why <file> [...] | --frame <file> <descriptors>\n");
  return 2;
}
