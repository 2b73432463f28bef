// PNG decoder in two halves, as jpeg_decode.h has for JPEG: the container and the serial entropy part (zlib inflate)
// on the caller's host thread, the per-pixel part (unfiltering, conversion to packed BGR, Adam7 placement) either on
// the device (csrc/kernels_png.hip, through ocr_png_frame) or here (pixels()).
//
// What comes out is what cv::imdecode(data, IMREAD_COLOR) returns, which is NOT what libpng's simplified API returns:
// OpenCV asks libpng for strip_16 (a 16-bit sample keeps its HIGH byte), strip_alpha (alpha is dropped, nothing is
// composited), expand_gray_1_2_4_to_8 (bit replication: x255, x85, x17), palette_to_rgb, gray_to_rgb and BGR order,
// and sets no gamma handling: gAMA / sRGB / iCCP / bKGD / tRNS do not change a pixel of the 3-channel result.  These
// rules, and the chunk-level ones below, are written from knowledge of libpng and OpenCV - neither source is on the
// build machine; tests/test_png_decode.py pins them against files built sample by sample and against Pillow.
//
//   - signature, then IHDR first (13 bytes): colour types 0, 2, 3, 4, 6 with their legal depths, compression and
//     filter method 0, interlace 0 or 1 (Adam7); width, height in 1 .. 2^31-1 and width * height <= 64 Mpixel, checked
//     before anything is allocated
//   - a critical chunk (IHDR, PLTE, IDAT, IEND) with a bad CRC, cut short, or of an unknown type refuses the file;
//     ancillary chunks are skipped unread, damaged or not (tRNS, gAMA, sRGB, iCCP, bKGD, eXIf among them)
//   - colour type 3 needs a PLTE of 1 .. 256 entries before the first IDAT; the table has 256 entries, zero beyond
//     PLTE, so an index past it is black (libpng's zeroed palette gives the same, from memory); PLTE in a grey file
//     is ignored
//   - the IDAT chunks are one zlib stream and follow one another: an IDAT after another chunk has come in between
//     refuses the file (libpng's "Too many IDATs found", from memory); the stream is read until IEND (a file without IEND
//     is cut short: refused)
//   - the stream must inflate to at least the bytes IHDR implies - the sum over the (non-empty) passes of
//     rows * (1 + rowbytes); fewer is libpng's "Not enough image data"; surplus is ignored
//   - a filter byte above 4 refuses the file
// zlib is resolved at run time (dlopen of libz.so.1): no link dependency.  available() says whether that worked; the
// caller keeps another PNG path for when it did not.
#pragma once
#include <dlfcn.h>

#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

namespace PaddleOCR {
namespace png {

constexpr long kMaxPixels = 64L << 20;  // the cap of the service's other decoders (kMaxDecodedPixels)
// What the device pixel stage takes; anything beyond is finished on the host (pixels()).  A header may claim a 1-pixel-wide
// image of 64M rows: a segment per row would be gigabytes of table for megabytes of pixels, and one segment of all of
// them a million bands on a single wave.  So: no more segments than this (the table is dropped, not grown), and no pass
// with more rows than kMaxDeviceRows (a segment is at most a pass: 256 bands).
constexpr size_t kMaxSegments = 1u << 16;
constexpr int kMaxDeviceRows = 1 << 14;

struct Pass {  // one Adam7 pass (the whole image when not interlaced): pixel (i, j) of it is image pixel (y0 + i*dy, x0 + j*dx)
  int x0 = 0, y0 = 0, dx = 1, dy = 1;
  int rows = 0, cols = 0;
  size_t rowbytes = 0;  // without the filter byte
  size_t offset = 0;    // of the pass's first filter byte in the inflated stream
};
// Maximal runs of rows of one pass that never look at a row outside the run: the first row of a pass, or a row whose
// filter is None or Sub, starts one.  The unit of parallel work on the device.
struct Segment { int32_t pass, first_row, rows; };

inline int channels_of(int color_type) { return color_type == 0 || color_type == 3 ? 1 : color_type == 4 ? 2 : color_type == 2 ? 3 : color_type == 6 ? 4 : 0; }
inline bool legal_format(int color_type, int depth) {
  switch (color_type) {
    case 0: return depth == 1 || depth == 2 || depth == 4 || depth == 8 || depth == 16;
    case 3: return depth == 1 || depth == 2 || depth == 4 || depth == 8;
    case 2: case 4: case 6: return depth == 8 || depth == 16;
    default: return false;
  }
}
// the passes of a width x height image (7 when interlaced, some possibly empty: rows or cols 0; else 1) and the size of
// the inflated stream; false when the header is not one this decoder takes
inline bool geometry(long width, long height, int depth, int color_type, int interlace, Pass pass[7], int& npass, size_t& total) {
  if (width <= 0 || height <= 0 || width > 0x7fffffffL || height > 0x7fffffffL || width * height > kMaxPixels) return false;
  if (!legal_format(color_type, depth) || (interlace != 0 && interlace != 1)) return false;
  static const int X0[7] = {0, 4, 0, 2, 0, 1, 0}, Y0[7] = {0, 0, 4, 0, 2, 0, 1}, DX[7] = {8, 8, 4, 4, 2, 2, 1}, DY[7] = {8, 8, 8, 4, 4, 2, 2};
  const size_t bits = (size_t)channels_of(color_type) * depth;
  npass = interlace ? 7 : 1;
  total = 0;
  for (int p = 0; p < npass; ++p) {
    Pass& q = pass[p];
    q = Pass();
    if (interlace) { q.x0 = X0[p]; q.y0 = Y0[p]; q.dx = DX[p]; q.dy = DY[p]; }
    q.cols = width > q.x0 ? (int)((width - q.x0 + q.dx - 1) / q.dx) : 0;
    q.rows = height > q.y0 ? (int)((height - q.y0 + q.dy - 1) / q.dy) : 0;
    if (q.cols == 0 || q.rows == 0) { q.cols = q.rows = 0; }
    q.rowbytes = ((size_t)q.cols * bits + 7) / 8;
    q.offset = total;
    if (q.rows) total += (size_t)q.rows * (1 + q.rowbytes);
  }
  return true;
}

struct Frame {
  int width = 0, height = 0, bit_depth = 0, color_type = 0, interlace = 0;
  uint8_t palette[768] = {};     // R, G, B x 256
  std::vector<uint8_t> data;     // the inflated stream, exactly the size geometry() gives
  std::vector<Segment> segments; // in stream order; they tile the rows of every non-empty pass.  Empty when !device_ok
  bool device_ok = false;        // within kMaxSegments / kMaxDeviceRows: the device pixel stage may take the frame
  int bpp() const { const int b = channels_of(color_type) * bit_depth; return b < 8 ? 1 : b / 8; }  // the filters' pixel distance
};

// ---- zlib, resolved at run time
struct ZStream {  // z_stream of zlib.h on an LP64 target
  const uint8_t* next_in; unsigned avail_in; unsigned long total_in;
  uint8_t* next_out; unsigned avail_out; unsigned long total_out;
  const char* msg; void* state; void* zalloc; void* zfree; void* opaque;
  int data_type; unsigned long adler, reserved;
};
struct Zlib {
  int (*init)(ZStream*, const char*, int) = nullptr;
  int (*inflate)(ZStream*, int) = nullptr;
  int (*end)(ZStream*) = nullptr;
  bool ok() const { return init && inflate && end; }
};
inline const Zlib& zlib() {
  static const Zlib z = [] {
    Zlib r;
    if (void* lib = dlopen("libz.so.1", RTLD_NOW | RTLD_LOCAL)) {
      r.init = (int (*)(ZStream*, const char*, int))dlsym(lib, "inflateInit_");
      r.inflate = (int (*)(ZStream*, int))dlsym(lib, "inflate");
      r.end = (int (*)(ZStream*))dlsym(lib, "inflateEnd");
    }
    return r;
  }();
  return z;
}
inline bool available() { return zlib().ok(); }

inline uint32_t crc32(const uint8_t* p, size_t n) {
  static const std::vector<uint32_t> table = [] {
    std::vector<uint32_t> t(256);
    for (uint32_t i = 0; i < 256; ++i) {
      uint32_t c = i;
      for (int k = 0; k < 8; ++k) c = (c & 1) ? 0xEDB88320u ^ (c >> 1) : c >> 1;
      t[i] = c;
    }
    return t;
  }();
  uint32_t c = 0xFFFFFFFFu;
  for (size_t i = 0; i < n; ++i) c = table[(c ^ p[i]) & 0xFF] ^ (c >> 8);
  return c ^ 0xFFFFFFFFu;
}

// Walks the filter byte of every scanline of f.data once: false on a value above 4; fills f.segments.
inline bool scan(Frame& f) {
  Pass pass[7];
  int npass;
  size_t total;
  if (!geometry(f.width, f.height, f.bit_depth, f.color_type, f.interlace, pass, npass, total) || f.data.size() < total) return false;
  f.segments.clear();
  f.device_ok = true;
  for (int p = 0; p < npass; ++p) {
    const Pass& q = pass[p];
    if (q.rows > kMaxDeviceRows) f.device_ok = false;
    const uint8_t* row = f.data.data() + q.offset;
    for (int r = 0; r < q.rows; ++r, row += 1 + q.rowbytes) {
      const uint8_t ft = row[0];
      if (ft > 4) return false;
      if (!f.device_ok) continue;  // (the filter bytes are still checked)
      if (r == 0 || ft <= 1) {
        if (f.segments.size() == kMaxSegments) f.device_ok = false;
        else f.segments.push_back(Segment{p, r, 1});
      } else f.segments.back().rows++;
    }
  }
  if (!f.device_ok) std::vector<Segment>().swap(f.segments);
  return true;
}

// The container and the inflate: everything but the pixels.  false = the file is refused (or zlib is missing).
inline bool parse(const uint8_t* d, size_t n, Frame& f) {
  static const uint8_t sig[8] = {0x89, 'P', 'N', 'G', 0x0D, 0x0A, 0x1A, 0x0A};
  if (n < 8 || memcmp(d, sig, 8) || !available()) return false;
  auto be32 = [&](size_t o) { return ((uint32_t)d[o] << 24) | ((uint32_t)d[o + 1] << 16) | ((uint32_t)d[o + 2] << 8) | (uint32_t)d[o + 3]; };
  size_t pos = 8;
  bool have_ihdr = false, have_plte = false, have_idat = false, have_iend = false, idat_closed = false;
  std::vector<std::pair<size_t, size_t>> idat;  // (offset, length) of every IDAT payload
  Pass pass[7];
  int npass = 0;
  size_t total = 0;
  f = Frame();
  while (!have_iend) {
    if (n - pos < 12) return false;  // the file ends without IEND
    const size_t len = be32(pos);
    const uint8_t* type = d + pos + 4;
    const bool critical = !(type[0] & 0x20);
    if (len > 0x7fffffffu || n - pos - 12 < len) return false;  // cut short (whatever the chunk: nothing after it can be read)
    const uint8_t* body = d + pos + 8;
    const bool crc_ok = crc32(type, 4 + len) == be32(pos + 8 + len);
    pos += 12 + len;
    if (!have_ihdr) {  // IHDR comes first
      if (memcmp(type, "IHDR", 4) || len != 13 || !crc_ok) return false;
      const uint32_t w = ((uint32_t)body[0] << 24) | (body[1] << 16) | (body[2] << 8) | body[3];
      const uint32_t h = ((uint32_t)body[4] << 24) | (body[5] << 16) | (body[6] << 8) | body[7];
      if (body[10] != 0 || body[11] != 0) return false;  // compression / filter method
      if (!geometry((long)w, (long)h, body[8], body[9], body[12], pass, npass, total)) return false;
      f.width = (int)w; f.height = (int)h; f.bit_depth = body[8]; f.color_type = body[9]; f.interlace = body[12];
      have_ihdr = true;
      continue;
    }
    if (have_idat && memcmp(type, "IDAT", 4)) idat_closed = true;  // (an ancillary chunk ends the run of IDATs too)
    if (!critical) continue;  // ancillary: unread, whatever its CRC says
    if (!crc_ok) return false;
    if (!memcmp(type, "IHDR", 4)) return false;
    else if (!memcmp(type, "PLTE", 4)) {
      if (have_plte || have_idat || len == 0 || len % 3 || len > 768) return false;
      have_plte = true;
      if (f.color_type & 2) memcpy(f.palette, body, len);  // (types 3, 2, 6; only 3 reads it.  A grey file's PLTE is ignored)
    } else if (!memcmp(type, "IDAT", 4)) {
      if ((f.color_type == 3 && !have_plte) || idat_closed) return false;
      have_idat = true;
      if (len) idat.emplace_back((size_t)(body - d), len);
    } else if (!memcmp(type, "IEND", 4)) {
      have_iend = true;
    } else {
      return false;  // a critical chunk this decoder does not know
    }
  }
  if (!have_idat) return false;
  // one zlib stream over the IDAT payloads, into a buffer that grows to - never beyond - what IHDR implies (a header
  // may claim half a gigabyte over a body of a few bytes: the claim alone allocates nothing)
  const Zlib& z = zlib();
  ZStream zs;
  memset(&zs, 0, sizeof zs);
  if (z.init(&zs, "1.2.11", (int)sizeof zs) != 0) return false;
  f.data.resize(total < (size_t)65536 ? total : (size_t)65536);
  size_t produced = 0, chunk = 0;
  bool ended = false, failed = false;
  while (produced < total && !ended && !failed) {
    if (zs.avail_in == 0) {
      if (chunk == idat.size()) break;  // the stream is cut short
      zs.next_in = d + idat[chunk].first;
      zs.avail_in = (unsigned)idat[chunk].second;
      ++chunk;
    }
    if (produced == f.data.size()) f.data.resize(f.data.size() * 2 < total ? f.data.size() * 2 : total);
    const size_t room = f.data.size() - produced;
    zs.next_out = f.data.data() + produced;
    zs.avail_out = (unsigned)(room < 0x40000000u ? room : 0x40000000u);
    const unsigned before = zs.avail_out;
    const int rc = z.inflate(&zs, 0 /* Z_NO_FLUSH */);
    produced += before - zs.avail_out;
    if (rc == 1 /* Z_STREAM_END */) ended = true;
    else if (rc != 0 && rc != -5 /* Z_BUF_ERROR: no progress possible right now */) failed = true;
    else if (rc == -5 && zs.avail_in != 0 && zs.avail_out != 0) failed = true;
  }
  z.end(&zs);
  if (produced < total) { f = Frame(); return false; }  // "Not enough image data" (surplus, if any, was never inflated)
  f.data.resize(total);
  if (!scan(f)) { f = Frame(); return false; }
  return true;
}

inline int paeth(int a, int b, int c) {
  const int p = a + b - c, pa = p > a ? p - a : a - p, pb = p > b ? p - b : b - p, pc = p > c ? p - c : c - p;
  return pa <= pb && pa <= pc ? a : pb <= pc ? b : c;
}

// The pixel half on the host: unfilter, convert, place.  bgr: height x width x 3.  false on a frame that parse() / scan()
// would not have produced.
inline bool pixels(const Frame& f, std::vector<uint8_t>& bgr) {
  Pass pass[7];
  int npass;
  size_t total;
  if (!geometry(f.width, f.height, f.bit_depth, f.color_type, f.interlace, pass, npass, total) || f.data.size() < total) return false;
  const int bpp = f.bpp(), depth = f.bit_depth, ct = f.color_type;
  const int step = depth == 16 ? 2 : 1;  // bytes per sample (the high byte comes first)
  bgr.assign((size_t)f.width * f.height * 3, 0);
  std::vector<uint8_t> cur, prev;
  for (int p = 0; p < npass; ++p) {
    const Pass& q = pass[p];
    if (!q.rows) continue;
    cur.assign(q.rowbytes, 0);
    prev.assign(q.rowbytes, 0);
    const uint8_t* row = f.data.data() + q.offset;
    for (int r = 0; r < q.rows; ++r, row += 1 + q.rowbytes) {
      const uint8_t ft = row[0];
      if (ft > 4) return false;
      for (size_t i = 0; i < q.rowbytes; ++i) {
        const int a = i >= (size_t)bpp ? cur[i - bpp] : 0, b = prev[i], c = i >= (size_t)bpp ? prev[i - bpp] : 0;
        const int pred = ft == 0 ? 0 : ft == 1 ? a : ft == 2 ? b : ft == 3 ? (a + b) >> 1 : paeth(a, b, c);
        cur[i] = (uint8_t)(row[1 + i] + pred);
      }
      uint8_t* out = bgr.data() + ((size_t)(q.y0 + (size_t)r * q.dy) * f.width + q.x0) * 3;
      for (int j = 0; j < q.cols; ++j, out += (size_t)q.dx * 3) {
        if (depth < 8) {  // grey or palette index, most significant bits first
          const int per = 8 / depth, v = (cur[j / per] >> ((per - 1 - j % per) * depth)) & ((1 << depth) - 1);
          if (ct == 3) { out[0] = f.palette[3 * v + 2]; out[1] = f.palette[3 * v + 1]; out[2] = f.palette[3 * v]; }
          else out[0] = out[1] = out[2] = (uint8_t)(v * (255 / ((1 << depth) - 1)));
        } else {
          const uint8_t* s = cur.data() + (size_t)j * bpp;
          if (ct == 3) { out[0] = f.palette[3 * s[0] + 2]; out[1] = f.palette[3 * s[0] + 1]; out[2] = f.palette[3 * s[0]]; }
          else if (ct & 2) { out[0] = s[2 * step]; out[1] = s[step]; out[2] = s[0]; }
          else out[0] = out[1] = out[2] = s[0];
        }
      }
      cur.swap(prev);
    }
  }
  return true;
}

}  // namespace png
}  // namespace PaddleOCR
