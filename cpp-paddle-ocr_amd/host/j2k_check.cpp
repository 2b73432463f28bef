// j2k_check: the JPEG 2000 decoder of j2k_decode.h (boxes, markers, tier-2, tier-1, host pixel stage) in one plain host
// process that links nothing of the library - what the tests compile with -fsanitize=address,undefined.  Every file is copied
// to a heap block of exactly its size, so a read past its end is the sanitizer's to see.
// j2k_check --decode <file> <out> [<file> <out> ...]: j2k::parse + j2k::pixels; out: the packed BGR image.  Prints
//   "<width> <height>" per file; the first refused file ends the run with exit status 1 and its reason on stderr.
// j2k_check --try <file> <out> [...]: as --decode, but a refused file prints "refused" (and writes nothing) and the run goes on.
// j2k_check --frame <file> <descriptors> [<file> <descriptors> ...]: j2k::parse, then the frame descriptor:
//   [i32 x 24: width, height, x0, y0, ncomp, prec, transform, mct, chan[3], device_ok, progression, layers, tiles_x, tiles_y,
//   file_comps, jp2, qstyle, cbw, cbh, precincts, tileparts, sop + 2 eph][u64 n][n tile-component records of 40 bytes
//   (j2k::TileComp)][u64 n][n float32 steps][u64 n][n int32 coefficients], little-endian.
// j2k_check --pixels <descriptors> <out>: j2k::pixels alone, over descriptors (any number, one after another) instead of files -
//   what the device stage is compared with; out: the BGR images one after another (nothing for a refused frame: the exit
//   status is 1 then).
// j2k_check --why <file> [...]: per file one line, "ok <width> <height>" or "refused: <reason>"; exit status 0.
// j2k_check --coded <file> <coded> [<file> <coded> ...]: j2k::parse_coded, then the coded descriptor - the frame before tier-1:
//   [i32 x 24 as for --frame][u64 n][n tile-component records][u64 n][n float32 steps][u64 ncoeffs: what tier-1 fills]
//   [u64 n][n code-block records of 32 bytes (j2k::CodedBlock)][u64 n][n bytes: the blocks' segments], little-endian.  A
//   refused file ends the run as for --frame.
// j2k_check --tier1 <coded> <descriptors>: j2k::tier1 over coded descriptors (any number, one after another); out: per
//   descriptor the frame in the form of --frame.  A descriptor that breaks a rule (j2k::fault_of, j2k::coded_fault) writes
//   nothing and prints "refused: <reason>" on stderr: the exit status is 1 then.
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <string>

#include "j2k_decode.h"

using namespace PaddleOCR;

static std::unique_ptr<uint8_t[]> read_file(const std::string& path, size_t& n) {
  FILE* f = fopen(path.c_str(), "rb");
  if (!f) { fprintf(stderr, "cannot read %s\n", path.c_str()); exit(2); }
  fseek(f, 0, SEEK_END);
  const long len = ftell(f);
  fseek(f, 0, SEEK_SET);
  if (len < 0) exit(2);
  std::unique_ptr<uint8_t[]> buf(new uint8_t[len ? len : 1]);
  if (fread(buf.get(), 1, (size_t)len, f) != (size_t)len) exit(2);
  fclose(f);
  n = (size_t)len;
  return buf;
}

static bool parse_path(const std::string& path, j2k::Frame& frame) {
  size_t len = 0;
  const std::unique_ptr<uint8_t[]> buf = read_file(path, len);
  return j2k::parse(buf.get(), len, frame);
}

static bool parse_coded_path(const std::string& path, j2k::Coded& cd) {
  size_t len = 0;
  const std::unique_ptr<uint8_t[]> buf = read_file(path, len);
  return j2k::parse_coded(buf.get(), len, cd);
}

static void write_head(FILE* o, const j2k::Frame& fr) {
  const int32_t head[24] = {fr.width, fr.height, fr.x0, fr.y0, fr.ncomp, fr.prec, fr.transform, fr.mct, fr.chan[0], fr.chan[1], fr.chan[2], fr.device_ok,
                            fr.progression, fr.layers, fr.tiles_x, fr.tiles_y, fr.file_comps, fr.jp2, fr.qstyle, fr.cbw, fr.cbh, fr.precincts, fr.tileparts,
                            fr.sop + 2 * fr.eph};
  fwrite(head, 1, sizeof head, o);
  uint64_t n = fr.tcs.size();
  fwrite(&n, 1, 8, o);
  fwrite(fr.tcs.data(), sizeof(j2k::TileComp), fr.tcs.size(), o);
  n = fr.steps.size();
  fwrite(&n, 1, 8, o);
  fwrite(fr.steps.data(), 4, fr.steps.size(), o);
}

static void write_frame(FILE* o, const j2k::Frame& fr) {
  write_head(o, fr);
  const uint64_t n = fr.coeffs.size();
  fwrite(&n, 1, 8, o);
  fwrite(fr.coeffs.data(), 4, fr.coeffs.size(), o);
}

static void write_coded(FILE* o, const j2k::Coded& cd) {
  write_head(o, cd.frame);
  uint64_t n = cd.ncoeffs;
  fwrite(&n, 1, 8, o);
  n = cd.cblks.size();
  fwrite(&n, 1, 8, o);
  fwrite(cd.cblks.data(), sizeof(j2k::CodedBlock), cd.cblks.size(), o);
  n = cd.bytes.size();
  fwrite(&n, 1, 8, o);
  fwrite(cd.bytes.data(), 1, cd.bytes.size(), o);
}

// head, tile-components and steps of a descriptor, as write_head wrote them; 0: the end of the file, 2: a broken one
static int read_head(FILE* f, j2k::Frame& fr) {
  int32_t head[24];
  const size_t got = fread(head, 1, sizeof head, f);
  if (got == 0) return 0;
  uint64_t n;
  if (got != sizeof head || fread(&n, 1, 8, f) != 8 || n > ((uint64_t)1 << 22)) return 2;
  fr.width = head[0]; fr.height = head[1]; fr.x0 = head[2]; fr.y0 = head[3]; fr.ncomp = head[4]; fr.prec = head[5]; fr.transform = head[6]; fr.mct = head[7];
  fr.chan[0] = head[8]; fr.chan[1] = head[9]; fr.chan[2] = head[10]; fr.device_ok = head[11] != 0;
  fr.progression = head[12]; fr.layers = head[13]; fr.tiles_x = head[14]; fr.tiles_y = head[15]; fr.file_comps = head[16]; fr.jp2 = head[17]; fr.qstyle = head[18];
  fr.cbw = head[19]; fr.cbh = head[20]; fr.precincts = head[21]; fr.tileparts = head[22]; fr.sop = head[23] & 1; fr.eph = head[23] >> 1;
  fr.tcs.resize((size_t)n);
  if (fread(fr.tcs.data(), sizeof(j2k::TileComp), (size_t)n, f) != n) return 2;
  if (fread(&n, 1, 8, f) != 8 || n > ((uint64_t)1 << 26)) return 2;
  fr.steps.resize((size_t)n);
  if (fread(fr.steps.data(), 4, (size_t)n, f) != n) return 2;
  return 1;
}

static int tier1_of_coded(const char* in, const char* outp) {
  FILE* f = fopen(in, "rb");
  FILE* o = fopen(outp, "wb");
  if (!f || !o) return 2;
  int rc = 0;
  for (;;) {
    j2k::Coded cd;
    j2k::Frame& fr = cd.frame;
    const int got = read_head(f, fr);
    if (got == 0) break;
    uint64_t n;
    if (got != 1 || fread(&n, 1, 8, f) != 8 || n > ((uint64_t)1 << 30)) return 2;
    cd.ncoeffs = (size_t)n;
    if (fread(&n, 1, 8, f) != 8 || n > ((uint64_t)1 << 26)) return 2;
    cd.cblks.resize((size_t)n);
    if (fread(cd.cblks.data(), sizeof(j2k::CodedBlock), (size_t)n, f) != n) return 2;
    if (fread(&n, 1, 8, f) != 8 || n > ((uint64_t)1 << 31)) return 2;
    cd.bytes.resize((size_t)n);
    if (fread(cd.bytes.data(), 1, (size_t)n, f) != n) return 2;
    const char* why = j2k::fault_of(fr.width, fr.height, fr.x0, fr.y0, fr.ncomp, fr.prec, fr.transform, fr.mct, fr.chan, fr.tcs.data(), fr.tcs.size(), fr.steps.size(), cd.ncoeffs);
    if (!why) why = j2k::coded_fault(fr.tcs.data(), fr.tcs.size(), cd.cblks.data(), cd.cblks.size(), cd.bytes.size());
    if (why) { fprintf(stderr, "refused: %s\n", why); rc = 1; continue; }
    fr.coeffs.resize(cd.ncoeffs);
    if (!j2k::tier1(cd, fr.coeffs.data())) return 2;
    write_frame(o, fr);
  }
  fclose(f);
  fclose(o);
  return rc;
}

static int pixels_of_frames(const char* in, const char* outp) {
  FILE* f = fopen(in, "rb");
  FILE* o = fopen(outp, "wb");
  if (!f || !o) return 2;
  int rc = 0;
  for (;;) {
    j2k::Frame fr;
    const int got = read_head(f, fr);
    if (got == 0) break;
    uint64_t n;
    if (got != 1 || fread(&n, 1, 8, f) != 8 || n > ((uint64_t)1 << 30)) return 2;
    fr.coeffs.resize((size_t)n);
    if (fread(fr.coeffs.data(), 4, (size_t)n, f) != n) return 2;
    std::vector<uint8_t> bgr;
    if (!j2k::pixels(fr, bgr)) { rc = 1; continue; }
    fwrite(bgr.data(), 1, bgr.size(), o);
  }
  fclose(f);
  fclose(o);
  return rc;
}

int main(int argc, char** argv) {
  const std::string mode = argc > 1 ? argv[1] : "";
  if (mode == "--pixels" && argc == 4) return pixels_of_frames(argv[2], argv[3]);
  if (mode == "--tier1" && argc == 4) return tier1_of_coded(argv[2], argv[3]);
  if (mode == "--coded" && argc >= 4 && argc % 2 == 0) {
    for (int i = 2; i < argc; i += 2) {
      j2k::Coded cd;
      if (!parse_coded_path(argv[i], cd)) { fprintf(stderr, "refused: %s: %s\n", argv[i], cd.frame.error ? cd.frame.error : "decode failure"); return 1; }
      FILE* o = fopen(argv[i + 1], "wb");
      if (!o) return 2;
      write_coded(o, cd);
      fclose(o);
    }
    return 0;
  }
  if (mode == "--why" && argc >= 3) {
    for (int i = 2; i < argc; ++i) {
      j2k::Frame frame;
      if (parse_path(argv[i], frame)) printf("ok %d %d\n", frame.width, frame.height);
      else printf("refused: %s\n", frame.error ? frame.error : "decode failure");
    }
    return 0;
  }
  if (mode == "--frame" && argc >= 4 && argc % 2 == 0) {
    for (int i = 2; i < argc; i += 2) {
      j2k::Frame frame;
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
      j2k::Frame frame;
      std::vector<uint8_t> bgr;
      if (!parse_path(argv[i], frame) || !j2k::pixels(frame, bgr)) {
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
  fprintf(stderr, "usage: j2k_check --decode|--try <file> <out> [...] | --frame <file> <descriptors> [...] | --pixels <descriptors> <out> | --why <file> [...] | --coded <file> <coded> [...] | --tier1 <coded> <descriptors>\n");
  return 2;
}
