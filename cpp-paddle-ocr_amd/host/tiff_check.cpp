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
// tiff_check --chunks <file> <out> [<file> <out> ...]: tiff::parse; out: Frame::data, the expanded chunks at their nominal size.
// tiff_check --coded <file> <out> [<file> <out> ...]: tiff::parse_coded; out: the Coded in a flat little-endian form - [i32 width, height,
//   photometric, bits, samples, planar, predictor, big_endian, premultiply, tile_width, tile_height][1024 palette bytes]
//   [i32 compression][u64 chunks][per chunk: u64 byte_off, u32 byte_len, u32 rows][u64 length][that many pool bytes].  Exit
//   status 1 for a refused file, 3 for one that takes the other route (Deflate).
// tiff_check --expand <in> <out>: tiff::expand over Codeds of that form, one after another; out: Frame::data of each (nothing
//   for a refused one: the exit status is 1 then) - what the device expansion is compared with.  Prints "ok" or "refused" per frame.
// tiff_check --why <file> [...]: per file "<file>: ok", "refused", "other route" or - a sound CCITT file - "fax" (parse_coded's answer).
// tiff_check --extents <streams> <out>: streams: repeated [u32 compression (5 or 32773), u32 need, u32 length][the bytes];
//   out: per stream two bytes, the verdict of lzw_extent / packbits_extent and that of unlzw / unpack_bits for the same need.
// tiff_check --route-deflate <file> <out> [...]: tiff::parse_deflate; out: the Coded in the form of --coded.  Exit status 1 for a
//   file that is refused or is not a Deflate one.
// tiff_check --inflate <streams> <out>: streams: repeated [u32 need, u32 length][the bytes]; out: per stream [u8 good][u32
//   produced][need bytes: what zlib wrote, zeros behind] - tiff::detail::inflate_count, the host's verdict the device's inflate
//   kernel is held to (and the form of inflate_check).  Prints "<streams> <good>".
// tiff_check --inflate-all <in> <out>: tiff::inflate_all over Codeds of that form; out and what is printed as --expand.
// tiff_check --route-fax <file> <out> [...]: tiff::parse_fax; out: the Coded in the form of --coded with [u32 T4Options] behind the
//   compression.  Exit status 1 for a file that is refused or is not a CCITT one; its reason goes to stderr.
// tiff_check --unfax <in> <out>: tiff::unfax_all over Codeds of that form; out as --expand; prints "ok" or "refused: <reason>" per
//   frame - what the device's fax expansion is compared with.
// tiff_check --fax-why <file> [...]: per file "<file>: <parse_fax's answer> | <parse's answer>", an answer being "ok", the reason
//   a rule of the coding refused the file with, or "refused" (the container did).
// tiff_check --fax-scan <streams> <out>: streams: repeated [u32 compression, T4Options, width, rows, length][the bytes]; out: per
//   stream two bytes, the verdict of ccitt::walk as the scan (no output) and as the decoder, into a block of exactly rows * row bytes.
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

static const char* const kRouteName[] = {"refused", "ok", "other route", "fax"};

static int coded_of_file(const char* in, const char* outp, bool deflate = false, bool fax = false) {
  std::unique_ptr<uint8_t[]> buf;
  size_t n = 0;
  if (!read_exact(in, buf, n)) { fprintf(stderr, "cannot read %s\n", in); return 2; }
  tiff::Coded c;
  if (fax) {
    const char* why = nullptr;
    if (!tiff::parse_fax(buf.get(), n, c, &why)) { fprintf(stderr, "refused: %s: %s\n", why ? why : "the container", in); return 1; }
  } else if (deflate) {
    if (!tiff::parse_deflate(buf.get(), n, c)) { fprintf(stderr, "refused: %s\n", in); return 1; }
  } else {
    const tiff::Route route = tiff::parse_coded(buf.get(), n, c);
    if (route != tiff::kCoded) { fprintf(stderr, "%s: %s\n", kRouteName[route], in); return route == tiff::kRefused ? 1 : 3; }
  }
  FILE* o = fopen(outp, "wb");
  if (!o) return 2;
  const tiff::Frame& f = c.frame;
  const int32_t head[11] = {f.width, f.height, f.photometric, f.bits, f.samples, f.planar, f.predictor, f.big_endian, f.premultiply, f.tile_width, f.tile_height};
  const int32_t comp = c.compression;
  const uint64_t nchunks = c.chunks.size(), len = c.bytes.size();
  fwrite(head, 1, sizeof head, o);
  fwrite(f.palette, 1, 1024, o);
  fwrite(&comp, 1, 4, o);
  if (fax) fwrite(&c.t4_options, 1, 4, o);
  fwrite(&nchunks, 1, 8, o);
  for (const tiff::Chunk& k : c.chunks) { fwrite(&k.byte_off, 1, 8, o); fwrite(&k.byte_len, 1, 4, o); fwrite(&k.rows, 1, 4, o); }
  fwrite(&len, 1, 8, o);
  fwrite(c.bytes.data(), 1, c.bytes.size(), o);
  fclose(o);
  printf("%d %d %d %zu %zu\n", f.width, f.height, c.compression, c.chunks.size(), c.bytes.size());
  return 0;
}

static int expand_codeds(const char* in, const char* outp, bool deflate = false, bool fax = false) {
  FILE* f = fopen(in, "rb");
  FILE* o = fopen(outp, "wb");
  if (!f || !o) return 2;
  int rc = 0;
  for (;;) {
    int32_t head[11], comp;
    uint64_t nchunks, len;
    tiff::Coded c;
    const size_t got = fread(head, 1, sizeof head, f);
    if (got == 0) break;
    if (got != sizeof head || fread(c.frame.palette, 1, 1024, f) != 1024 || fread(&comp, 1, 4, f) != 4 || (fax && fread(&c.t4_options, 1, 4, f) != 4) ||
        fread(&nchunks, 1, 8, f) != 8) return 2;
    tiff::Frame& fr = c.frame;
    fr.width = head[0]; fr.height = head[1]; fr.photometric = head[2]; fr.bits = head[3]; fr.samples = head[4];
    fr.planar = head[5]; fr.predictor = head[6]; fr.big_endian = head[7]; fr.premultiply = head[8];
    fr.tile_width = head[9]; fr.tile_height = head[10];
    c.compression = comp;
    if (nchunks > ((uint64_t)1 << 24)) return 2;
    c.chunks.resize((size_t)nchunks);
    for (tiff::Chunk& k : c.chunks)
      if (fread(&k.byte_off, 1, 8, f) != 8 || fread(&k.byte_len, 1, 4, f) != 4 || fread(&k.rows, 1, 4, f) != 4) return 2;
    if (fread(&len, 1, 8, f) != 8 || len > ((uint64_t)1 << 31)) return 2;
    // (a heap block of exactly the pool's size: a read past it is the sanitizer's to see)
    std::unique_ptr<uint8_t[]> pool(new uint8_t[len ? len : 1]);
    if (fread(pool.get(), 1, (size_t)len, f) != len) return 2;
    c.bytes.assign(pool.get(), pool.get() + len);
    c.bytes.shrink_to_fit();
    tiff::Frame out;
    if (fax) {
      const char* why = nullptr;
      if (!tiff::unfax_all(c, out, &why)) { rc = 1; printf("refused: %s\n", why ? why : "?"); continue; }
      printf("ok\n");
      fwrite(out.data.data(), 1, out.data.size(), o);
      continue;
    }
    if (!(deflate ? tiff::inflate_all(c, out) : tiff::expand(c, out))) { rc = 1; printf("refused\n"); continue; }
    printf("ok\n");
    fwrite(out.data.data(), 1, out.data.size(), o);
  }
  fclose(f);
  fclose(o);
  return rc;
}

static int extents_of_streams(const char* in, const char* outp) {
  FILE* f = fopen(in, "rb");
  FILE* o = fopen(outp, "wb");
  if (!f || !o) return 2;
  for (;;) {
    uint32_t head[3];
    const size_t got = fread(head, 1, sizeof head, f);
    if (got == 0) break;
    if (got != sizeof head || head[1] > (1u << 26) || head[2] > (1u << 26)) return 2;
    const size_t need = head[1], len = head[2];
    std::unique_ptr<uint8_t[]> s(new uint8_t[len ? len : 1]), out(new uint8_t[need ? need : 1]);  // exactly their sizes
    if (fread(s.get(), 1, len, f) != len) return 2;
    uint8_t verdict[2];
    if (head[0] == 5) { verdict[0] = tiff::detail::lzw_extent(s.get(), len, need); verdict[1] = tiff::detail::unlzw(s.get(), len, out.get(), need); }
    else { verdict[0] = tiff::detail::packbits_extent(s.get(), len, need); verdict[1] = tiff::detail::unpack_bits(s.get(), len, out.get(), need); }
    fwrite(verdict, 1, 2, o);
  }
  fclose(f);
  fclose(o);
  return 0;
}

static int fax_scan_streams(const char* in, const char* outp) {
  FILE* f = fopen(in, "rb");
  FILE* o = fopen(outp, "wb");
  if (!f || !o) return 2;
  for (;;) {
    uint32_t head[5];
    const size_t got = fread(head, 1, sizeof head, f);
    if (got == 0) break;
    if (got != sizeof head || head[2] < 1 || head[2] > (1u << 20) || head[3] > (1u << 16) || head[4] > (1u << 26)) return 2;
    const size_t len = head[4], row_bytes = (head[2] + 7) / 8, need = row_bytes * head[3];
    std::unique_ptr<uint8_t[]> s(new uint8_t[len ? len : 1]), out(new uint8_t[need ? need : 1]);  // exactly their sizes
    if (fread(s.get(), 1, len, f) != len) return 2;
    memset(out.get(), 0, need);
    const uint8_t verdict[2] = {!ccitt::walk(s.get(), len, (int)head[0], head[1], head[2], head[3], nullptr, 0),
                                !ccitt::walk(s.get(), len, (int)head[0], head[1], head[2], head[3], out.get(), row_bytes)};
    fwrite(verdict, 1, 2, o);
  }
  fclose(f);
  fclose(o);
  return 0;
}

static int inflate_streams(const char* in, const char* outp) {
  FILE* f = fopen(in, "rb");
  FILE* o = fopen(outp, "wb");
  if (!f || !o) return 2;
  long streams = 0, good = 0;
  for (;;) {
    uint32_t head[2];
    const size_t got = fread(head, 1, sizeof head, f);
    if (got == 0) break;
    if (got != sizeof head || head[0] > (1u << 26) || head[1] > (1u << 26)) return 2;
    const size_t need = head[0], len = head[1];
    std::unique_ptr<uint8_t[]> s(new uint8_t[len ? len : 1]), out(new uint8_t[need ? need : 1]);  // exactly their sizes
    if (fread(s.get(), 1, len, f) != len) return 2;
    memset(out.get(), 0, need);
    const uint32_t produced = (uint32_t)tiff::detail::inflate_count(s.get(), len, out.get(), need);
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
  if (mode == "--coded" && argc >= 4 && argc % 2 == 0) {
    for (int i = 2; i < argc; i += 2)
      if (const int rc = coded_of_file(argv[i], argv[i + 1])) return rc;
    return 0;
  }
  if (mode == "--chunks" && argc >= 4 && argc % 2 == 0) {
    for (int i = 2; i < argc; i += 2) {
      std::unique_ptr<uint8_t[]> buf;
      size_t n = 0;
      if (!read_exact(argv[i], buf, n)) { fprintf(stderr, "cannot read %s\n", argv[i]); return 2; }
      tiff::Frame frame;
      if (!tiff::parse(buf.get(), n, frame)) { fprintf(stderr, "refused: %s\n", argv[i]); return 1; }
      FILE* o = fopen(argv[i + 1], "wb");
      if (!o) return 2;
      fwrite(frame.data.data(), 1, frame.data.size(), o);
      fclose(o);
    }
    return 0;
  }
  if (mode == "--expand" && argc == 4) return expand_codeds(argv[2], argv[3]);
  if (mode == "--inflate-all" && argc == 4) return expand_codeds(argv[2], argv[3], true);
  if (mode == "--inflate" && argc == 4) return inflate_streams(argv[2], argv[3]);
  if (mode == "--route-deflate" && argc >= 4 && argc % 2 == 0) {
    for (int i = 2; i < argc; i += 2)
      if (const int rc = coded_of_file(argv[i], argv[i + 1], true)) return rc;
    return 0;
  }
  if (mode == "--route-fax" && argc >= 4 && argc % 2 == 0) {
    for (int i = 2; i < argc; i += 2)
      if (const int rc = coded_of_file(argv[i], argv[i + 1], false, true)) return rc;
    return 0;
  }
  if (mode == "--unfax" && argc == 4) return expand_codeds(argv[2], argv[3], false, true);
  if (mode == "--fax-scan" && argc == 4) return fax_scan_streams(argv[2], argv[3]);
  if (mode == "--fax-why" && argc >= 3) {
    for (int i = 2; i < argc; ++i) {
      std::unique_ptr<uint8_t[]> buf;
      size_t n = 0;
      if (!read_exact(argv[i], buf, n)) { fprintf(stderr, "cannot read %s\n", argv[i]); return 2; }
      tiff::Coded c;
      tiff::Frame frame;
      const char *scan = nullptr, *full = nullptr;
      const bool a = tiff::parse_fax(buf.get(), n, c, &scan), b = tiff::parse(buf.get(), n, frame, &full);
      printf("%s: %s | %s\n", argv[i], a ? "ok" : scan ? scan : "refused", b ? "ok" : full ? full : "refused");
    }
    return 0;
  }
  if (mode == "--extents" && argc == 4) return extents_of_streams(argv[2], argv[3]);
  if (mode == "--why" && argc >= 3) {
    for (int i = 2; i < argc; ++i) {
      std::unique_ptr<uint8_t[]> buf;
      size_t n = 0;
      if (!read_exact(argv[i], buf, n)) { fprintf(stderr, "cannot read %s\n", argv[i]); return 2; }
      tiff::Coded c;
      printf("%s: %s\n", argv[i], kRouteName[tiff::parse_coded(buf.get(), n, c)]);
    }
    return 0;
  }
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
  fprintf(stderr, "usage: tiff_check --decode <file> <out> [...] | --pixels <descriptors> <out> | --reject <dir> | --chunks <file> <out> [...] | --coded <file> <out> [...] | --expand <codeds> <out> | "
                  "--why <file> [...] | --extents <streams> <out> | --route-deflate <file> <out> [...] | --inflate <streams> <out> | --inflate-all <codeds> <out> | "
                  "--route-fax <file> <out> [...] | --unfax <codeds> <out> | --fax-why <file> [...] | --fax-scan <streams> <out>\n");
  return 2;
}
