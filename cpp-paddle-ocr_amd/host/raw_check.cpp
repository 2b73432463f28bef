// raw_check <bundle>: the BMP / PNM decoder of raw_decode.h (container, run-length and ASCII expansion, host pixel stage)
// over many inputs in one plain host process that links nothing of the library - what the tests compile with
// -fsanitize=address,undefined.  bundle: repeated [u32 little-endian length][that many bytes of a (possibly hostile)
// file].  Every input is copied to a heap block of exactly its size, so a read past its end is the sanitizer's to see.
// Prints "accepted <n> refused <m> checksum <of the accepted images' pixels>" and a line "verdicts " + one A or R per
// input; exit status 0 unless the bundle itself is malformed.
// raw_check --pixels <frames> <out>: raw::pixels alone, over frame descriptors instead of files - what the device stage is
// compared with.  frames: repeated [i32 width, height, kind, bottom_up][u64 row_stride][1024 palette bytes][u64 length]
// [that many bytes of stored rows], little-endian; out: the BGR images one after another (nothing for a refused frame: the
// exit status is 1 then).
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <string>

#include "raw_decode.h"

static int pixels_of_frames(const char* in, const char* outp) {
  FILE* f = fopen(in, "rb");
  FILE* o = fopen(outp, "wb");
  if (!f || !o) return 2;
  int rc = 0;
  for (;;) {
    int32_t head[4];
    uint64_t stride, len;
    PaddleOCR::raw::Frame frame;
    const size_t got = fread(head, 1, sizeof head, f);
    if (got == 0) break;
    if (got != sizeof head || fread(&stride, 1, 8, f) != 8 || fread(frame.palette, 1, 1024, f) != 1024 || fread(&len, 1, 8, f) != 8) return 2;
    frame.width = head[0]; frame.height = head[1]; frame.kind = head[2]; frame.bottom_up = head[3]; frame.row_stride = (size_t)stride;
    frame.data.resize((size_t)len);
    if (fread(frame.data.data(), 1, (size_t)len, f) != len) return 2;
    std::vector<uint8_t> bgr;
    if (!PaddleOCR::raw::pixels(frame, bgr)) { rc = 1; continue; }
    fwrite(bgr.data(), 1, bgr.size(), o);
  }
  fclose(f);
  fclose(o);
  return rc;
}

int main(int argc, char** argv) {
  if (argc == 4 && std::string(argv[1]) == "--pixels") return pixels_of_frames(argv[2], argv[3]);
  if (argc != 2) { fprintf(stderr, "usage: raw_check <bundle>\n"); return 2; }
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  long accepted = 0, refused = 0;
  unsigned long sum = 0;
  std::string verdicts;
  for (;;) {
    uint8_t l[4];
    const size_t got = fread(l, 1, 4, f);
    if (got == 0) break;
    if (got != 4) return 2;
    const size_t n = (size_t)l[0] | ((size_t)l[1] << 8) | ((size_t)l[2] << 16) | ((size_t)l[3] << 24);
    std::unique_ptr<uint8_t[]> buf(new uint8_t[n ? n : 1]);
    if (fread(buf.get(), 1, n, f) != n) return 2;
    PaddleOCR::raw::Frame frame;
    std::vector<uint8_t> bgr;
    if (PaddleOCR::raw::parse(buf.get(), n, frame) && PaddleOCR::raw::pixels(frame, bgr)) {
      ++accepted;
      verdicts += 'A';
      for (uint8_t b : bgr) sum = sum * 31 + b;
    } else {
      ++refused;
      verdicts += 'R';
    }
  }
  fclose(f);
  printf("accepted %ld refused %ld checksum %lu\nverdicts %s\n", accepted, refused, sum, verdicts.c_str());
  return 0;
}
