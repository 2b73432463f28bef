// BMP and PNM (PBM / PGM / PPM) decoders in two halves, shaped like png_decode.h: the container and whatever is serial
// (run-length expansion, ASCII number parsing) on the caller's host thread - parse() - and the per-pixel part (bit and
// nibble unpacking, palette, 5-5-5 / 5-6-5 expansion, high bytes of 16-bit samples, row order, channel order) either on
// the device (csrc/kernels_raw.hip, through ocr_raw_frame) or here - pixels().
//
// What comes out is what cv::imdecode(data, IMREAD_COLOR) returns.  No OpenCV source or binary is on the build machine:
// the rules are restated from memory of modules/imgcodecs/src/grfmt_bmp.cpp and grfmt_pxm.cpp (OpenCV 4.x) - DESIGN.md
// section 5 lists each one as unpinned and says where the memory is unsure; tests/test_raw_decode.py pins them against
// files built sample by sample (tests/raw_writer.py) and, where Pillow agrees by design, against Pillow.
//
// BMP
//   - "BM", header of 12 (OS/2 core: 16-bit unsigned width and height, 3-byte palette entries), 40, 52, 56, 108 or 124
//     bytes; width > 0, height != 0, negative height = rows stored top-down (uncompressed and BITFIELDS only), else bottom-up
//   - 1, 4, 8, 16, 24, 32 bits per pixel; compression 0, 1 (RLE8, 8 bpp), 2 (RLE4, 4 bpp), 3 (BITFIELDS, 16 / 32 bpp)
//   - palette: biClrUsed entries (1 << bpp when 0, clamped to that), B,G,R,x; entries the file does not have, and indices
//     past the palette, are 0
//   - 16 bpp: 5-5-5, or with BITFIELDS the masks 7C00/03E0/001F (5-5-5) or F800/07E0/001F (5-6-5), any other triple
//     refused; expansion by shifting, the low bits stay 0
//   - 32 bpp: B,G,R,A with A dropped; BITFIELDS masks are skipped, not interpreted
//   - rows padded to 4 bytes; every row must be in the file (the last one may lack its padding)
//   - RLE8 / RLE4 are expanded HERE into one index byte per pixel over a canvas of index 0: 00 00 end of line, 00 01 end of
//     bitmap, 00 02 dx dy move, absolute runs padded to 16 bits, runs clipped at the row end, a stream that ends early
//     keeps what it has, a move or run that leaves the canvas ends the decode
// PNM
//   - P1 .. P6 (P7 refused); whitespace and # comments between the header fields, one whitespace byte before binary data;
//     maxval 1 .. 65535 (none for P1 / P4)
//   - P1 / P4: bit 1 is black; P4 rows padded to a byte, most significant bit first; P2 / P5 grey to B = G = R; P3 / P6
//     R,G,B to B,G,R; maxval <= 255: the sample as it is (no rescaling); above: two bytes big-endian, the HIGH byte kept
//   - ASCII forms are parsed HERE into the binary sample array (a value above maxval becomes maxval; P1 reads one digit
//     per sample); running out of numbers refuses the file
// Every size is checked against the bytes present before anything is allocated; width * height <= 64 Mpixel.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

namespace PaddleOCR {
namespace raw {

constexpr long kMaxPixels = 64L << 20;  // the cap of the service's other decoders (kMaxDecodedPixels)

enum Kind {  // ocr_raw_kind of include/ocr_hip.h, value for value
  INDEX1, INDEX4, INDEX8, BGR555, BGR565, BGR24, BGRX32, RGB24, GREY8, GREY16BE, RGB48BE, BIT1_INV, kKinds
};
// bytes of a stored row of `width` pixels, without padding
inline size_t row_bytes(int kind, size_t width) {
  switch (kind) {
    case INDEX1: case BIT1_INV: return (width + 7) / 8;
    case INDEX4: return (width + 1) / 2;
    case INDEX8: case GREY8: return width;
    case BGR555: case BGR565: case GREY16BE: return width * 2;
    case BGR24: case RGB24: return width * 3;
    case BGRX32: return width * 4;
    case RGB48BE: return width * 6;
    default: return 0;
  }
}

struct Frame {
  int width = 0, height = 0, kind = 0;
  int bottom_up = 0;           // stored row r is image row height - 1 - r
  size_t row_stride = 0;       // bytes between stored rows
  uint8_t palette[1024] = {};  // B,G,R,x times 256, zero beyond the file's
  std::vector<uint8_t> data;   // the stored rows: (height - 1) * row_stride + row_bytes(kind, width) bytes at least
};

namespace detail {

inline uint32_t le16(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8); }
inline uint32_t le32(const uint8_t* p) { return le16(p) | (le16(p + 2) << 16); }

// RLE8 (nibbles = false) / RLE4 into canvas (width x height index bytes, stored-row order, zeroed by the caller)
inline void rle_expand(const uint8_t* s, size_t n, bool nibbles, int width, int height, uint8_t* canvas) {
  long x = 0, y = 0;
  size_t i = 0;
  while (n - i >= 2 && y < height) {
    const int c = s[i], v = s[i + 1];
    i += 2;
    if (c > 0) {  // encoded run, clipped at the row end
      uint8_t* row = canvas + (size_t)y * width;
      for (int k = 0; k < c && x < width; ++k, ++x) row[x] = nibbles ? (uint8_t)((k & 1) ? v & 15 : v >> 4) : (uint8_t)v;
    } else if (v == 0) {
      x = 0; ++y;
    } else if (v == 1) {
      return;
    } else if (v == 2) {
      if (n - i < 2) return;
      x += s[i]; y += s[i + 1];
      i += 2;
      if (x > width) return;  // (y is checked by the loop)
    } else {  // absolute run of v pixels, padded to 16 bits
      const size_t bytes = nibbles ? ((size_t)v + 1) / 2 : (size_t)v, have = n - i < bytes ? n - i : bytes;
      uint8_t* row = canvas + (size_t)y * width;
      for (int k = 0; k < v && x < width; ++k, ++x) {
        const size_t b = nibbles ? (size_t)k / 2 : (size_t)k;
        if (b >= have) return;  // the stream ends inside the run
        row[x] = nibbles ? (uint8_t)((k & 1) ? s[i + b] & 15 : s[i + b] >> 4) : s[i + b];
      }
      if (have < bytes) return;
      i += (bytes + 1) & ~(size_t)1;
      if (i > n) return;
    }
  }
}

inline bool parse_bmp(const uint8_t* d, size_t n, Frame& f) {
  if (n < 26 || d[0] != 'B' || d[1] != 'M') return false;
  const size_t off = le32(d + 10);
  const uint32_t hdr = le32(d + 14);
  if (hdr != 12 && hdr != 40 && hdr != 52 && hdr != 56 && hdr != 108 && hdr != 124) return false;
  if (n < 14 + (size_t)hdr) return false;
  long w, hs;
  unsigned bpp, comp = 0, used = 0;
  if (hdr == 12) {
    w = (long)le16(d + 18); hs = (long)le16(d + 20); bpp = le16(d + 24);
  } else {
    w = (int32_t)le32(d + 18); hs = (int32_t)le32(d + 22); bpp = le16(d + 28); comp = le32(d + 30); used = le32(d + 46);
  }
  if (w <= 0 || hs == 0 || hs == INT32_MIN) return false;
  const long h = hs < 0 ? -hs : hs;
  if (w * h > kMaxPixels) return false;  // (w, h < 2^31: no overflow in 64 bits)
  if (bpp != 1 && bpp != 4 && bpp != 8 && bpp != 16 && bpp != 24 && bpp != 32) return false;
  if (!(comp == 0 || (comp == 1 && bpp == 8) || (comp == 2 && bpp == 4) || (comp == 3 && (bpp == 16 || bpp == 32)))) return false;
  if ((comp == 1 || comp == 2) && hs < 0) return false;  // a run-length stream has no top-down form
  if (off > n) return false;
  f = Frame();
  f.width = (int)w; f.height = (int)h; f.bottom_up = hs > 0;
  if (bpp <= 8) {
    const size_t pal = 14 + (size_t)hdr, entry = hdr == 12 ? 3 : 4;
    size_t count = used ? used : (size_t)1 << bpp;
    if (count > ((size_t)1 << bpp)) count = (size_t)1 << bpp;
    if (count > (n - pal) / entry) count = (n - pal) / entry;
    for (size_t k = 0; k < count; ++k) memcpy(f.palette + 4 * k, d + pal + entry * k, 3);
  }
  bool is565 = false;
  if (bpp == 16 && comp == 3) {  // the three masks sit at byte 54, behind a 40-byte header or inside a longer one
    if (n < 66) return false;
    const uint32_t r = le32(d + 54), g = le32(d + 58), b = le32(d + 62);
    if (r == 0xF800 && g == 0x07E0 && b == 0x001F) is565 = true;
    else if (!(r == 0x7C00 && g == 0x03E0 && b == 0x001F)) return false;
  }
  if (comp == 1 || comp == 2) {
    f.kind = INDEX8;
    f.row_stride = (size_t)w;
    f.data.assign((size_t)w * h, 0);
    rle_expand(d + off, n - off, comp == 2, (int)w, (int)h, f.data.data());
    return true;
  }
  f.kind = bpp == 1 ? INDEX1 : bpp == 4 ? INDEX4 : bpp == 8 ? INDEX8 : bpp == 16 ? (is565 ? BGR565 : BGR555) : bpp == 24 ? BGR24 : BGRX32;
  f.row_stride = (((size_t)w * bpp + 31) / 32) * 4;
  const size_t need = (size_t)(h - 1) * f.row_stride + row_bytes(f.kind, (size_t)w);  // <= 64M * 4 + 4: no overflow
  if (n - off < need) return false;
  f.data.assign(d + off, d + off + need);
  return true;
}

// whitespace and comments, then a decimal number of at most `digits` digits; false at the end of the bytes or on a foreign byte
inline bool pnm_number(const uint8_t* d, size_t n, size_t& i, long& out, int digits = 32) {
  for (;;) {
    while (i < n && (d[i] == ' ' || d[i] == '\n' || d[i] == '\r' || d[i] == '\t' || d[i] == '\v' || d[i] == '\f')) ++i;
    if (i < n && d[i] == '#') { while (i < n && d[i] != '\n') ++i; continue; }
    break;
  }
  if (i >= n || d[i] < '0' || d[i] > '9') return false;
  long x = 0;
  for (int k = 0; k < digits && i < n && d[i] >= '0' && d[i] <= '9'; ++k, ++i)
    if (x <= 1000000) x = x * 10 + (d[i] - '0');  // (beyond any legal field: stays large, never overflows)
  out = x;
  return true;
}

inline bool parse_pnm(const uint8_t* d, size_t n, Frame& f) {
  if (n < 3 || d[0] != 'P' || d[1] < '1' || d[1] > '6') return false;
  const int type = d[1] - '0';
  const bool bits = type == 1 || type == 4, ascii = type <= 3;
  size_t i = 2;
  long w, h, maxval = 1;
  if (!pnm_number(d, n, i, w) || !pnm_number(d, n, i, h) || (!bits && !pnm_number(d, n, i, maxval))) return false;
  if (w <= 0 || h <= 0 || w > 1000000 || h > 1000000 || w * h > kMaxPixels || maxval < 1 || maxval > 65535) return false;
  const bool wide = maxval > 255;
  const int channels = (type == 3 || type == 6) ? 3 : 1;
  f = Frame();
  f.width = (int)w; f.height = (int)h;
  f.kind = bits ? BIT1_INV : channels == 1 ? (wide ? GREY16BE : GREY8) : (wide ? RGB48BE : RGB24);
  f.row_stride = row_bytes(f.kind, (size_t)w);
  const size_t total = f.row_stride * (size_t)h;  // <= 64M * 6
  if (!ascii) {
    ++i;  // the single whitespace byte after the header
    if (i > n || n - i < total) return false;
    f.data.assign(d + i, d + i + total);
    return true;
  }
  // ASCII: a sample takes a digit at least, and a separator too where values may have several digits
  const size_t samples = (size_t)w * h * channels, left = n - i;
  if (bits ? left < samples : left + 1 < 2 * samples) return false;
  f.data.assign(total, 0);
  for (long y = 0; y < h; ++y) {
    uint8_t* row = f.data.data() + (size_t)y * f.row_stride;
    for (size_t k = 0; k < (size_t)w * channels; ++k) {
      long v;
      if (!pnm_number(d, n, i, v, bits ? 1 : 32)) { f = Frame(); return false; }
      if (bits) { if (v != 0) row[k >> 3] |= (uint8_t)(0x80 >> (k & 7)); continue; }
      if (v > maxval) v = maxval;
      if (wide) { row[2 * k] = (uint8_t)(v >> 8); row[2 * k + 1] = (uint8_t)v; }
      else row[k] = (uint8_t)v;
    }
  }
  return true;
}

}  // namespace detail

// The container and the serial part: everything but the pixels.  false = not a BMP / PNM file, or one that is refused.
inline bool parse(const uint8_t* d, size_t n, Frame& f) {
  if (n >= 2 && d[0] == 'B' && d[1] == 'M') return detail::parse_bmp(d, n, f);
  if (n >= 2 && d[0] == 'P') return detail::parse_pnm(d, n, f);
  return false;
}

// what the descriptor of a frame must satisfy (the rules of csrc/capi_raw.hip's check, on this side of the ABI)
inline bool sound(const Frame& f) {
  if (f.kind < 0 || f.kind >= kKinds || f.width <= 0 || f.height <= 0 || (long)f.width * f.height > kMaxPixels) return false;
  const size_t rb = row_bytes(f.kind, (size_t)f.width);
  if (f.row_stride < rb || f.row_stride > ((size_t)1 << 31)) return false;  // (times height < 2^26: no overflow below)
  return f.data.size() >= (size_t)(f.height - 1) * f.row_stride + rb;
}

// The pixel half on the host.  bgr: height x width x 3.  false on a frame that parse() would not have produced.
inline bool pixels(const Frame& f, std::vector<uint8_t>& bgr) {
  if (!sound(f)) return false;
  const int w = f.width, h = f.height;
  bgr.resize((size_t)w * h * 3);
  for (int y = 0; y < h; ++y) {
    const uint8_t* s = f.data.data() + (size_t)(f.bottom_up ? h - 1 - y : y) * f.row_stride;
    uint8_t* o = bgr.data() + (size_t)y * w * 3;
    for (int x = 0; x < w; ++x, o += 3) {
      switch (f.kind) {
        case INDEX1: memcpy(o, f.palette + 4 * ((s[x >> 3] >> (7 - (x & 7))) & 1), 3); break;
        case INDEX4: memcpy(o, f.palette + 4 * ((x & 1) ? s[x >> 1] & 15 : s[x >> 1] >> 4), 3); break;
        case INDEX8: memcpy(o, f.palette + 4 * s[x], 3); break;
        case BGR555: { const unsigned t = s[2 * x] | (s[2 * x + 1] << 8); o[0] = (uint8_t)(t << 3); o[1] = (uint8_t)((t >> 2) & 0xF8); o[2] = (uint8_t)((t >> 7) & 0xF8); } break;
        case BGR565: { const unsigned t = s[2 * x] | (s[2 * x + 1] << 8); o[0] = (uint8_t)(t << 3); o[1] = (uint8_t)((t >> 3) & 0xFC); o[2] = (uint8_t)((t >> 8) & 0xF8); } break;
        case BGR24: memcpy(o, s + 3 * (size_t)x, 3); break;
        case BGRX32: memcpy(o, s + 4 * (size_t)x, 3); break;
        case RGB24: o[0] = s[3 * (size_t)x + 2]; o[1] = s[3 * (size_t)x + 1]; o[2] = s[3 * (size_t)x]; break;
        case GREY8: o[0] = o[1] = o[2] = s[x]; break;
        case GREY16BE: o[0] = o[1] = o[2] = s[2 * (size_t)x]; break;
        case RGB48BE: o[0] = s[6 * (size_t)x + 4]; o[1] = s[6 * (size_t)x + 2]; o[2] = s[6 * (size_t)x]; break;
        default: o[0] = o[1] = o[2] = ((s[x >> 3] >> (7 - (x & 7))) & 1) ? 0 : 255; break;  // BIT1_INV
      }
    }
  }
  return true;
}

}  // namespace raw
}  // namespace PaddleOCR
