// vp8_check: the lossy WebP decoder of vp8_decode.h (container hand-over, boolean decoder, headers, modes, tokens, host pixel
// stage) in one plain host process that links nothing of the library - what the tests compile with
// -fsanitize=address,undefined.  Every file is copied to a heap block of exactly its size, so a read past its end is the
// sanitizer's to see.
// vp8_check --decode <file> <out> [<file> <out> ...]: vp8::parse_file + vp8::pixels; out: the packed BGR image.  Prints
//   "<width> <height>" per file; the first refused file ends the run with exit status 1 and its reason on stderr.
// vp8_check --try <file> <out> [...]: as --decode, but a refused file prints "refused" (and writes nothing) and the run goes on.
// vp8_check --frame <file> <descriptors> [<file> <descriptors> ...]: vp8::parse_file, then the frame descriptor:
//   [i32 width, height, filter_type, partitions, segments][u64 n][n macroblock records of 40 bytes (vp8::Mb)][u64 n][n int16
//   coefficients], little-endian.
// vp8_check --pixels <descriptors> <out>: vp8::pixels alone, over descriptors (any number, one after another) instead of files -
//   what the device stage is compared with; out: the BGR images one after another (nothing for a refused frame: the exit
//   status is 1 then).
// vp8_check --why <file> [...]: per file one line, "ok <width> <height>" or "refused: <reason>"; exit status 0.
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <string>

#include "vp8_decode.h"

using namespace PaddleOCR;

static bool parse_path(const std::string& path, vp8::Frame& frame) {
  FILE* f = fopen(path.c_str(), "rb");
  if (!f) { fprintf(stderr, "cannot read %s\n", path.c_str()); exit(2); }
  fseek(f, 0, SEEK_END);
  const long len = ftell(f);
  fseek(f, 0, SEEK_SET);
  if (len < 0) exit(2);
  std::unique_ptr<uint8_t[]> buf(new uint8_t[len ? len : 1]);
  if (fread(buf.get(), 1, (size_t)len, f) != (size_t)len) exit(2);
  fclose(f);
  return vp8::parse_file(buf.get(), (size_t)len, frame);
}

static void write_frame(FILE* o, const vp8::Frame& fr) {
  const int32_t head[5] = {fr.width, fr.height, fr.filter_type, fr.partitions, fr.segments};
  fwrite(head, 1, sizeof head, o);
  uint64_t n = fr.mbs.size();
  fwrite(&n, 1, 8, o);
  fwrite(fr.mbs.data(), sizeof(vp8::Mb), fr.mbs.size(), o);
  n = fr.coeffs.size();
  fwrite(&n, 1, 8, o);
  fwrite(fr.coeffs.data(), 2, fr.coeffs.size(), o);
}

static int pixels_of_frames(const char* in, const char* outp) {
  FILE* f = fopen(in, "rb");
  FILE* o = fopen(outp, "wb");
  if (!f || !o) return 2;
  int rc = 0;
  for (;;) {
    int32_t head[5];
    vp8::Frame fr;
    const size_t got = fread(head, 1, sizeof head, f);
    if (got == 0) break;
    uint64_t n;
    if (got != sizeof head || fread(&n, 1, 8, f) != 8 || n > ((uint64_t)1 << 22)) return 2;
    fr.width = head[0]; fr.height = head[1]; fr.filter_type = head[2];
    fr.mbs.resize((size_t)n);
    if (fread(fr.mbs.data(), sizeof(vp8::Mb), (size_t)n, f) != n) return 2;
    if (fread(&n, 1, 8, f) != 8 || n > ((uint64_t)1 << 30)) return 2;
    fr.coeffs.resize((size_t)n);
    if (fread(fr.coeffs.data(), 2, (size_t)n, f) != n) return 2;
    std::vector<uint8_t> bgr;
    if (!vp8::pixels(fr, bgr)) { rc = 1; continue; }
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
      vp8::Frame frame;
      if (parse_path(argv[i], frame)) printf("ok %d %d\n", frame.width, frame.height);
      else printf("refused: %s\n", frame.error ? frame.error : "decode failure");
    }
    return 0;
  }
  if (mode == "--frame" && argc >= 4 && argc % 2 == 0) {
    for (int i = 2; i < argc; i += 2) {
      vp8::Frame frame;
      if (!parse_path(argv[i], frame)) { fprintf(stderr, "refused: %s: %s\n", argv[i], frame.error ? frame.error : "decode failure"); return 1; }
      FILE* o = fopen(argv[i + 1], "wb");
      if (!o) return 2;
      write_frame(o, frame);
      fclose(o);
    }
    return 0;
  }
  if ((mode == "--decode" || mode == "--try") && argc >= 4 && argc % 2 == 0) {
    for (int i = 2; i < argc; i += 2) {
      vp8::Frame frame;
      std::vector<uint8_t> bgr;
      if (!parse_path(argv[i], frame) || !vp8::pixels(frame, bgr)) {
        if (mode == "--try") { printf("refused\n"); continue; }
        fprintf(stderr, "refused: %s: %s\n", argv[i], frame.error ? frame.error : "decode failure");
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
  fprintf(stderr, "usage: vp8_check --decode|--try <file> <out> [...] | --frame <file> <descriptors> [...] | --pixels <descriptors> <out> | --why <file> [...]\n");
  return 2;
}
