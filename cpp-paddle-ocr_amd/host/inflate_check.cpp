// inflate_check: the walk of csrc/inflate_core.h - the very text of the device's inflate kernel - compiled as plain C++ for a
// "wavefront" of one lane, in one host process that links nothing of the library: what the tests build with
// -fsanitize=address,undefined.  Every stream and every output lie in heap blocks of exactly their sizes.
// inflate_check <streams> <out>: streams: repeated [u32 need, u32 length][the bytes]; out: per stream [u8 good (produced ==
//   need)][u32 produced][need bytes: what was written, zeros behind] - the form of tiff_check --inflate, which gives zlib's
//   answer to the same streams.  Prints "<streams> <good>".
#include <cstdio>
#include <cstring>
#include <memory>

#include "../csrc/inflate_core.h"

int main(int argc, char** argv) {
  if (argc != 3) { fprintf(stderr, "usage: inflate_check <streams> <out>\n"); return 2; }
  FILE* f = fopen(argv[1], "rb");
  FILE* o = fopen(argv[2], "wb");
  if (!f || !o) return 2;
  std::unique_ptr<ocr::inflate_core::Shared> sh(new ocr::inflate_core::Shared);
  long streams = 0, good = 0;
  for (;;) {
    uint32_t head[2];
    const size_t got = fread(head, 1, sizeof head, f);
    if (got == 0) break;
    if (got != sizeof head || head[0] > (1u << 26) || head[1] > (1u << 26)) return 2;
    const uint32_t need = head[0], len = head[1];
    std::unique_ptr<uint8_t[]> s(new uint8_t[len ? len : 1]), out(new uint8_t[need ? need : 1]);
    if (fread(s.get(), 1, len, f) != len) return 2;
    memset(out.get(), 0, need);
    memset(sh.get(), 0xA5, sizeof *sh);  // (nothing may rest on what an earlier stream left)
    ocr::inflate_core::Walk walk(*sh, ocr::inflate_core::Stream{s.get(), len, out.get(), need});
    const uint32_t produced = walk.run();
    if (produced > need) return 3;
    const uint8_t ok = produced == need;
    fwrite(&ok, 1, 1, o);
    fwrite(&produced, 1, 4, o);
    fwrite(out.get(), 1, need, o);
    ++streams;
    good += ok;
  }
  fclose(f);
  fclose(o);
  printf("%ld %ld\n", streams, good);
  return 0;
}
