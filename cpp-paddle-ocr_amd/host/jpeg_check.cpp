// jpeg_check: the JPEG decoder of jpeg_decode.h (markers, Huffman scans, host pixel stage) in one plain host process that links
// nothing of the library - what the tests compile with -fsanitize=address,undefined.  Every file is copied to a heap block of
// exactly its size, so a read past its end is the sanitizer's to see.
// jpeg_check --frame <file> <descriptors> [<file> <descriptors> ...]: Decoder::decode_coefficients, then the descriptor that
//   jpeg::Coefs holds (what ocr_jpeg_frame carries):
//   [i32 rows, cols, ncomp, orientation, color, reserved] and per component [i32 h, v, bw, bh, dw, dh][64 u16 quant, natural
//   order][u64 n][n int16 coefficients], little-endian.  A refused file ends the run with exit status 1.
// jpeg_check --pixels <descriptors> <out>: Decoder::pixels alone, over descriptors (any number, one after another) instead of
//   files - what the device stage is compared with; out: the oriented BGR images one after another.  A descriptor that breaks a
//   rule of ocr_jpeg_frame (include/ocr_hip.h) ends the run with exit status 1: Decoder::pixels trusts its input.
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <string>

#include "jpeg_decode.h"

using namespace PaddleOCR;

static bool coefs_of_path(const std::string& path, jpeg::Coefs& out) {
  FILE* f = fopen(path.c_str(), "rb");
  if (!f) { fprintf(stderr, "cannot read %s\n", path.c_str()); exit(2); }
  fseek(f, 0, SEEK_END);
  const long len = ftell(f);
  fseek(f, 0, SEEK_SET);
  if (len < 0) exit(2);
  std::unique_ptr<uint8_t[]> buf(new uint8_t[len ? len : 1]);
  if (fread(buf.get(), 1, (size_t)len, f) != (size_t)len) exit(2);
  fclose(f);
  jpeg::Decoder d;
  return d.decode_coefficients(buf.get(), (size_t)len, out);
}

static void write_frame(FILE* o, const jpeg::Coefs& c) {
  const int32_t head[6] = {c.rows, c.cols, c.ncomp, c.orientation, c.color, 0};
  fwrite(head, 1, sizeof head, o);
  for (int i = 0; i < c.ncomp; ++i) {
    const jpeg::Coefs::Comp& k = c.comp[i];
    const int32_t ch[6] = {k.h, k.v, k.bw, k.bh, k.dw, k.dh};
    fwrite(ch, 1, sizeof ch, o);
    fwrite(k.quant, 2, 64, o);
    const uint64_t n = k.coef.size();
    fwrite(&n, 1, 8, o);
    fwrite(k.coef.data(), 2, k.coef.size(), o);
  }
}

// the rules of ocr_jpeg_frame, as far as Decoder::pixels relies on them
static const char* fault_of(const jpeg::Coefs& c) {
  if (c.rows <= 0 || c.cols <= 0 || (long)c.rows * c.cols > (64L << 20)) return "size outside 1 .. 64 Mpixel";
  if (c.ncomp != 1 && c.ncomp != 3 && c.ncomp != 4) return "ncomp must be 1, 3 or 4";
  if (c.orientation < 0 || c.orientation > 8) return "orientation outside 0..8";
  const bool color_ok = c.ncomp == 1 ? c.color == jpeg::kGrey : c.ncomp == 3 ? (c.color == jpeg::kYCbCr || c.color == jpeg::kRGB)
                                                                              : (c.color == jpeg::kCMYK || c.color == jpeg::kYCCK);
  if (!color_ok) return "colour space does not fit the number of components";
  for (int i = 0; i < c.ncomp; ++i) {
    const jpeg::Coefs::Comp& k = c.comp[i];
    if (k.h < 1 || k.h > 4 || k.v < 1 || k.v > 4) return "sampling factor outside 1..4";
    if (c.hmax % k.h != 0 || c.vmax % k.v != 0) return "fractional upsampling";
    if (k.bw <= 0 || k.bh <= 0 || k.bw > 16384 || k.bh > 16384) return "block counts";
    if (k.dw != (int)(((long)c.cols * k.h + c.hmax - 1) / c.hmax) || k.dh != (int)(((long)c.rows * k.v + c.vmax - 1) / c.vmax)) return "dw / dh";
    if ((long)k.bw * 8 < k.dw || (long)k.bh * 8 < k.dh) return "the blocks do not cover the component";
    if (k.coef.size() != (size_t)k.bw * k.bh * 64) return "coefficient count is not bw * bh * 64";
  }
  return nullptr;
}

static int pixels_of_frames(const char* in, const char* outp) {
  FILE* f = fopen(in, "rb");
  FILE* o = fopen(outp, "wb");
  if (!f || !o) return 2;
  for (;;) {
    int32_t head[6];
    const size_t got = fread(head, 1, sizeof head, f);
    if (got == 0) break;
    if (got != sizeof head || head[2] < 1 || head[2] > 4) return 2;
    jpeg::Coefs c;
    c.rows = head[0]; c.cols = head[1]; c.ncomp = head[2]; c.orientation = head[3]; c.color = head[4];
    for (int i = 0; i < c.ncomp; ++i) {
      jpeg::Coefs::Comp& k = c.comp[i];
      int32_t ch[6];
      uint64_t n;
      if (fread(ch, 1, sizeof ch, f) != sizeof ch || fread(k.quant, 2, 64, f) != 64 || fread(&n, 1, 8, f) != 8 || n > ((uint64_t)1 << 30)) return 2;
      k.h = ch[0]; k.v = ch[1]; k.bw = ch[2]; k.bh = ch[3]; k.dw = ch[4]; k.dh = ch[5];
      k.coef.resize((size_t)n);
      if (fread(k.coef.data(), 2, (size_t)n, f) != n) return 2;
      if (k.h > c.hmax) c.hmax = k.h;
      if (k.v > c.vmax) c.vmax = k.v;
    }
    if (c.orientation == 0) c.orientation = 1;
    if (const char* fault = fault_of(c)) { fprintf(stderr, "refused: %s\n", fault); return 1; }
    std::vector<uint8_t> bgr;
    int rows = 0, cols = 0;
    if (!jpeg::Decoder::pixels(c, bgr, rows, cols) || rows != c.out_rows() || cols != c.out_cols()) return 1;
    fwrite(bgr.data(), 1, bgr.size(), o);
  }
  fclose(f);
  fclose(o);
  return 0;
}

int main(int argc, char** argv) {
  const std::string mode = argc > 1 ? argv[1] : "";
  if (mode == "--pixels" && argc == 4) return pixels_of_frames(argv[2], argv[3]);
  if (mode == "--frame" && argc >= 4 && argc % 2 == 0) {
    for (int i = 2; i < argc; i += 2) {
      jpeg::Coefs c;
      if (!coefs_of_path(argv[i], c)) { fprintf(stderr, "refused: %s\n", argv[i]); return 1; }
      FILE* o = fopen(argv[i + 1], "wb");
      if (!o) return 2;
      write_frame(o, c);
      fclose(o);
    }
    return 0;
  }
  fprintf(stderr, "usage: jpeg_check --frame <file> <descriptors> [...] | --pixels <descriptors> <out>\n");
  return 2;
}
