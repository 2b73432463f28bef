// tiff_check: the TIFF decoder of tiff_decode.h (container, PackBits / LZW / Deflate expansion, host pixel stage) in one
// plain host process that links nothing of the library - what the tests compile with -fsanitize=address,undefined.  Every
// file is copied to a heap block of exactly its size, so a read past its end is the sanitizer's to see.
// tiff_check --decode <file> <out> [<file> <out> ...]: tiff::parse + tiff::pixels; out: the packed BGR image.  Prints
//   "<width> <height>" per file; the first refused file ends the run with exit status 1.
// tiff_check --pixels <descriptors> <out>: tiff::pixels alone, over frame descriptors instead of files - what the device stage
//   is compared with.  descriptors: repeated [i32 width, height, photometric, bits, samples, planar, predictor, big_endian,
//   premultiply, tile_width, tile_height][1024 palette bytes][u64 length][that many bytes of expanded chunks], little-endian;
//   out: the BGR images one after another (nothing for a refused frame: the exit status is 1 then).
// tiff_check --reject <dir>: every file of the directory must be refused; prints "refused <n> accepted <m>" and the names
//   of the accepted ones; exit status 1 when there are any.
#include <dirent.h>

#include <cstdio>
#include <cstdlib>
#include <memory>
#include <string>

#include "tiff_decode.h"

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

static bool decode_file(const std::string& path, tiff::Frame& frame, std::vector<uint8_t>& bgr) {
  std::unique_ptr<uint8_t[]> buf;
  size_t n = 0;
  if (!read_exact(path, buf, n)) { fprintf(stderr, "cannot read %s\n", path.c_str()); exit(2); }
  return tiff::parse(buf.get(), n, frame) && tiff::pixels(frame, bgr);
}

static int pixels_of_frames(const char* in, const char* outp) {
  FILE* f = fopen(in, "rb");
  FILE* o = fopen(outp, "wb");
  if (!f || !o) return 2;
  int rc = 0;
  for (;;) {
    int32_t head[11];
    uint64_t len;
    tiff::Frame frame;
    const size_t got = fread(head, 1, sizeof head, f);
    if (got == 0) break;
    if (got != sizeof head || fread(frame.palette, 1, 1024, f) != 1024 || fread(&len, 1, 8, f) != 8) return 2;
    frame.width = head[0]; frame.height = head[1]; frame.photometric = head[2]; frame.bits = head[3]; frame.samples = head[4];
    frame.planar = head[5]; frame.predictor = head[6]; frame.big_endian = head[7]; frame.premultiply = head[8];
    frame.tile_width = head[9]; frame.tile_height = head[10];
    frame.data.resize((size_t)len);
    if (fread(frame.data.data(), 1, (size_t)len, f) != len) return 2;
    std::vector<uint8_t> bgr;
    if (!tiff::pixels(frame, bgr)) { rc = 1; continue; }
    fwrite(bgr.data(), 1, bgr.size(), o);
  }
  fclose(f);
  fclose(o);
  return rc;
}

static int reject_dir(const char* dir) {
  DIR* d = opendir(dir);
  if (!d) return 2;
  long refused = 0, accepted = 0;
  std::string names;
  while (const dirent* e = readdir(d)) {
    if (e->d_name[0] == '.') continue;
    tiff::Frame frame;
    std::vector<uint8_t> bgr;
    if (decode_file(std::string(dir) + "/" + e->d_name, frame, bgr)) { ++accepted; names += std::string(" ") + e->d_name; }
    else ++refused;
  }
  closedir(d);
  printf("refused %ld accepted %ld%s\n", refused, accepted, names.c_str());
  return accepted ? 1 : 0;
}

int main(int argc, char** argv) {
  const std::string mode = argc > 1 ? argv[1] : "";
  if (mode == "--pixels" && argc == 4) return pixels_of_frames(argv[2], argv[3]);
  if (mode == "--reject" && argc == 3) return reject_dir(argv[2]);
  if (mode == "--decode" && argc >= 4 && argc % 2 == 0) {
    for (int i = 2; i < argc; i += 2) {
      tiff::Frame frame;
      std::vector<uint8_t> bgr;
      if (!decode_file(argv[i], frame, bgr)) { fprintf(stderr, "refused: %s\n", argv[i]); return 1; }
      FILE* o = fopen(argv[i + 1], "wb");
      if (!o) return 2;
      fwrite(bgr.data(), 1, bgr.size(), o);
      fclose(o);
      printf("%d %d\n", frame.width, frame.height);
    }
    return 0;
  }
  fprintf(stderr, "usage: tiff_check --decode <file> <out> [...] | --pixels <descriptors> <out> | --reject <dir>\n");
  return 2;
}
