// png_check <bundle>: the PNG decoder of png_decode.h (container, inflate, host pixel stage) over many inputs in one
// plain host process that links nothing of the library - what the tests compile with -fsanitize=address,undefined.
// bundle: repeated [u32 little-endian length][that many bytes of a (possibly damaged) file].  Every input is copied to a
// heap block of exactly its size, so a read past its end is the sanitizer's to see.  Prints "accepted <n> refused <m>
// checksum <of the accepted images' pixels>" and a line "verdicts " + one A or R per input; exit status 0 unless the
// bundle itself is malformed.
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <string>

#include "png_decode.h"

int main(int argc, char** argv) {
  if (argc != 2) { fprintf(stderr, "usage: png_check <bundle>\n"); return 2; }
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
    PaddleOCR::png::Frame frame;
    std::vector<uint8_t> bgr;
    if (PaddleOCR::png::parse(buf.get(), n, frame) && PaddleOCR::png::pixels(frame, bgr)) {
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
