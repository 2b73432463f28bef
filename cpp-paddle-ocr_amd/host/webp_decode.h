// Lossless WebP (VP8L) decoder in two halves, shaped like png_decode.h / tiff_decode.h: the container and whatever is serial
// (prefix codes, LZ77, the colour cache) on the caller's host thread - parse() - and the pixel part (the inverse transforms:
// spatial predictor, cross-colour, add-green, palette with pixel bundling) either on the device (csrc/kernels_webp.hip,
// through ocr_webp_frame) or here - pixels().
//
// What comes out is what cv::imdecode(data, IMREAD_COLOR) returns: the pixels of libwebp's WebPDecodeBGR (alpha dropped, not
// applied).  tests/test_webp_decode.py compares every branch with the system's libwebp.
//
// Container: "RIFF" size "WEBP", then either a "VP8L" chunk or a "VP8X" chunk followed by any chunks, of which the first
// "VP8L" is the image ("ICCP", "EXIF", "XMP " and unknown chunks are skipped: libwebp ignores them, the ICC profile is not
// applied).  The RIFF size and every chunk size are checked against the bytes present; odd-sized chunks are padded.  A file
// whose VP8X flags say animation, or that holds "ANIM" / "ANMF", is refused with kNotLossless.  A file whose image is a lossy
// "VP8 " chunk (with or without "ALPH" in front, which is skipped) is not parse()'s either - it answers kNotLossless - but the
// chunk's payload and the VP8X canvas are handed over in Frame::vp8 for vp8_decode.h, which decodes it.
// VP8L: signature 0x2f, 14 bits width - 1, 14 bits height - 1, alpha_is_used (read, ignored), version 0; width * height
// <= 64 Mpixel.  Bits are read from the least significant bit of each byte on; a prefix code's bits arrive most significant
// first (as in Deflate).  Reading a bit the chunk does not have refuses the file.
//   - transforms: at most four, each kind once (a repeat is refused); block bits 2 .. 9; the predictor-mode and the
//     colour-multiplier sub-images and the palette are nested entropy-coded images without transforms of their own; the
//     palette is delta-coded, 1 .. 256 entries, and narrows the coded image to ceil(width / {8, 4, 2, 1}) for <= 2 / <= 4 /
//     <= 16 / more colours
//   - an entropy-coded image: an optional colour cache of 1 .. 11 bits, an optional (main image only) meta prefix image with
//     prefix bits 2 .. 9, five prefix codes per group (green + length + cache, red, blue, alpha, distance).  A code is simple
//     (1 or 2 symbols; one symbol costs no bits) or normal (code-length code in the fixed order, repeats 16 / 17 / 18,
//     max_symbol).  A code without symbols, an over-subscribed one and an incomplete one with more than one symbol are refused
//     (libwebp's rule: a single symbol of any length is a zero-bit code)
//   - LZ77: length and distance as prefix + extra bits, distances 1 .. 120 through the short-distance map (at least 1), a
//     distance before the start or a length past the end refuses the file; copies may overlap and run across rows
//   - every literal, cached and copied pixel enters the colour cache, hash (argb * 0x1e35a7bd) >> (32 - bits)
// Inverse transforms (pixels(), last in the file first), all sums per byte modulo 256:
//   - predictor: pixel (0, 0) adds 0xff000000; the rest of the top row adds L; the left column adds T; elsewhere the block's
//     mode m = (sub-image pixel >> 8) & 15: 0 black 0xff000000, 1 L, 2 T, 3 TR, 4 TL, 5 avg(avg(L, TR), T), 6 avg(L, TL),
//     7 avg(L, T), 8 avg(TL, T), 9 avg(T, TR), 10 avg(avg(L, TL), avg(T, TR)), 11 Select, 12 ClampAddSubtractFull,
//     13 ClampAddSubtractHalf, 14 and 15 black.  avg is per byte, rounded down, no carry between channels.  TR of the
//     rightmost pixel is the leftmost pixel of the CURRENT row (the pixel that follows in memory).  Select: T when the
//     Manhattan distance over the four channels |L - TL| is at most |T - TL|, else L.  Full: clamp(L + T - TL) per channel.
//     Half: with a = avg(L, T), clamp(a + (a - TL) / 2), C's division (towards zero)
//   - cross-colour, per block multipliers g2r = byte 0, g2b = byte 1, r2b = byte 2 of the sub-image pixel, as int8:
//     red += (g2r * (int8)green) >> 5; blue += (g2b * (int8)green) >> 5; blue += (r2b * (int8)red') >> 5 with the NEW red
//   - add-green: red += green, blue += green
//   - colour indexing: the green byte holds 8 / 4 / 2 / 1 indices, lowest bits first; an index beyond the palette is
//     transparent black
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <vector>

namespace PaddleOCR {
namespace webp {

constexpr long kMaxPixels = 64L << 20;  // the cap of the service's other decoders
constexpr int kMaxTransforms = 4;
enum Kind { PREDICTOR = 0, CROSS_COLOUR = 1, ADD_GREEN = 2, COLOUR_INDEXING = 3 };
// what a refused lossy or animated file is answered with
constexpr const char* kNotLossless = "lossy or animated WebP is not decoded (animated files, and lossy data without a key frame)";

struct Transform {
  int kind = 0;
  int bits = 0;  // predictor, cross-colour: a block is 2^bits square; colour indexing: a coded pixel holds 2^bits indices
  std::vector<uint32_t> data;  // predictor / cross-colour: the sub-image, ceil(w / 2^bits) x ceil(h / 2^bits); indexing: the palette
};

struct Frame {  // ocr_webp_frame of include/ocr_hip.h, field for field
  int width = 0, height = 0;
  std::vector<uint32_t> argb;          // the entropy-decoded image, coded_width(frame) x height
  std::vector<Transform> transforms;   // in file order; pixels() undoes them last to first
  bool device_ok = false;              // colour indexing, if present, is the file's first transform: the device stage may take it
  const char* error = nullptr;         // why parse() refused
  // a refused file whose image is a lossy "VP8 " chunk: its payload (inside the caller's bytes), and the VP8X canvas or 0 x 0
  const uint8_t* vp8 = nullptr;
  size_t vp8_size = 0;
  int canvas_width = 0, canvas_height = 0;
};

inline int ceil_shift(int v, int bits) { return (v + (1 << bits) - 1) >> bits; }
inline int index_bits(size_t colours) { return colours > 16 ? 0 : colours > 4 ? 1 : colours > 2 ? 2 : 3; }
// the width the transform at position t of the file works on: the full width in front of colour indexing, the coded one behind
inline int width_at(const Frame& f, size_t t) {
  int w = f.width;
  for (size_t k = 0; k < t && k < f.transforms.size(); ++k)
    if (f.transforms[k].kind == COLOUR_INDEXING) w = ceil_shift(w, f.transforms[k].bits & 3);
  return w;
}
inline int coded_width(const Frame& f) { return width_at(f, f.transforms.size()); }

// why pixels() (and the device stage, which states the same rules over ocr_webp_frame) refuses a frame; nullptr when sound
inline const char* fault(const Frame& f) {
  if (f.width <= 0 || f.height <= 0 || f.width > 16384 || f.height > 16384 || (long)f.width * f.height > kMaxPixels)
    return "webp frame: width and height must be 1 .. 16384 and at most 64 Mpixel together";
  if (f.transforms.size() > (size_t)kMaxTransforms) return "webp frame: at most four transforms";
  unsigned seen = 0;
  for (size_t t = 0; t < f.transforms.size(); ++t) {
    const Transform& tr = f.transforms[t];
    if (tr.kind < 0 || tr.kind > 3) return "webp frame: transform kind must be 0 .. 3";
    if (seen & (1u << tr.kind)) return "webp frame: a transform kind occurs twice";
    seen |= 1u << tr.kind;
    const int w = width_at(f, t);
    if (tr.kind == PREDICTOR || tr.kind == CROSS_COLOUR) {
      if (tr.bits < 2 || tr.bits > 9) return "webp frame: block bits must be 2 .. 9";
      if (tr.data.size() < (size_t)ceil_shift(w, tr.bits) * ceil_shift(f.height, tr.bits)) return "webp frame: a transform's sub-image is smaller than its blocks";
    } else if (tr.kind == ADD_GREEN) {
      if (tr.bits != 0) return "webp frame: add-green has no bits";
    } else {
      if (tr.data.empty() || tr.data.size() > 256) return "webp frame: the palette has 1 .. 256 entries";
      if (tr.bits != index_bits(tr.data.size())) return "webp frame: the bundling bits do not follow from the palette size";
    }
  }
  if (f.argb.size() < (size_t)coded_width(f) * f.height) return "webp frame: fewer coded pixels than coded width x height";
  return nullptr;
}
inline bool device_scope(const Frame& f) {
  for (size_t t = 1; t < f.transforms.size(); ++t)
    if (f.transforms[t].kind == COLOUR_INDEXING) return false;
  return true;
}

// ---------------------------------------------------------------------------------------------------------- the serial half
namespace detail {

struct Bits {
  const uint8_t* p;
  size_t n, pos = 0;
  uint64_t val = 0;
  int have = 0;
  bool eos = false;  // a bit beyond the data was asked for
  Bits(const uint8_t* d, size_t len) : p(d), n(len) {}
  void fill() {
    while (have <= 56 && pos < n) { val |= (uint64_t)p[pos++] << have; have += 8; }
  }
  uint32_t read(int k) {  // k <= 32
    if (k == 0) return 0;
    fill();
    if (have < k) { eos = true; have = 0; val = 0; return 0; }
    const uint32_t v = (uint32_t)(val & (((uint64_t)1 << k) - 1));
    val >>= k;
    have -= k;
    return v;
  }
};

// a canonical prefix code: symbols sorted by (length, value), decoded length by length; a table over the next 8 bits in front
struct Code {
  uint16_t count[16] = {};
  std::vector<uint16_t> sym;
  std::vector<uint16_t> fast;  // [next 8 bits, first bit lowest] -> length << 12 | symbol; 0: longer than 8 bits
  int single = -1;             // the code's only symbol: costs no bits

  bool build(const uint8_t* len, int n, bool want_fast) {
    int total = 0;
    for (int s = 0; s < n; ++s) { count[len[s]]++; total += len[s] != 0; }
    count[0] = 0;
    if (total == 0) return false;
    if (total == 1) {
      for (int s = 0; s < n; ++s) if (len[s]) single = s;
      return true;
    }
    int left = 1;
    for (int l = 1; l <= 15; ++l) {
      left = (left << 1) - count[l];
      if (left < 0) return false;  // over-subscribed
    }
    if (left != 0) return false;   // incomplete
    uint16_t offs[16], next[16];
    offs[1] = 0; next[1] = 0;
    for (int l = 1; l < 15; ++l) { offs[l + 1] = (uint16_t)(offs[l] + count[l]); next[l + 1] = (uint16_t)((next[l] + count[l]) << 1); }
    sym.resize((size_t)total);
    if (want_fast) fast.assign(256, 0);
    for (int s = 0; s < n; ++s) {
      const int l = len[s];
      if (!l) continue;
      sym[offs[l]++] = (uint16_t)s;
      const unsigned code = next[l]++;
      if (want_fast && l <= 8) {
        unsigned rev = 0;
        for (int b = 0; b < l; ++b) rev |= ((code >> b) & 1u) << (l - 1 - b);
        for (unsigned k = rev; k < 256; k += 1u << l) fast[k] = (uint16_t)((l << 12) | s);
      }
    }
    return true;
  }
  int read(Bits& br) const {
    if (single >= 0) return single;
    if (!fast.empty()) {
      br.fill();
      const uint16_t e = fast[br.val & 0xFF];
      if (e) {
        const int l = e >> 12;
        if (br.have < l) { br.eos = true; br.have = 0; br.val = 0; return e & 0xFFF; }
        br.val >>= l;
        br.have -= l;
        return e & 0xFFF;
      }
    }
    int code = 0, first = 0, index = 0;
    for (int l = 1; l <= 15; ++l) {
      code |= (int)br.read(1);
      const int c = count[l];
      if (code - c < first) return sym[(size_t)(index + (code - first))];
      index += c;
      first = (first + c) << 1;
      code <<= 1;
    }
    br.eos = true;  // (a complete code ends within 15 bits: not reached)
    return 0;
  }
};

// the 120 short distances: (dy << 4) | (8 - dx)
constexpr uint8_t kShort[120] = {
    0x18, 0x07, 0x17, 0x19, 0x28, 0x06, 0x27, 0x29, 0x16, 0x1a, 0x26, 0x2a, 0x38, 0x05, 0x37, 0x39, 0x15, 0x1b, 0x36, 0x3a, 0x25, 0x2b, 0x48, 0x04,
    0x47, 0x49, 0x14, 0x1c, 0x35, 0x3b, 0x46, 0x4a, 0x24, 0x2c, 0x58, 0x45, 0x4b, 0x34, 0x3c, 0x03, 0x57, 0x59, 0x13, 0x1d, 0x56, 0x5a, 0x23, 0x2d,
    0x44, 0x4c, 0x55, 0x5b, 0x33, 0x3d, 0x68, 0x02, 0x67, 0x69, 0x12, 0x1e, 0x66, 0x6a, 0x22, 0x2e, 0x54, 0x5c, 0x43, 0x4d, 0x65, 0x6b, 0x32, 0x3e,
    0x78, 0x01, 0x77, 0x79, 0x53, 0x5d, 0x11, 0x1f, 0x64, 0x6c, 0x42, 0x4e, 0x76, 0x7a, 0x21, 0x2f, 0x75, 0x7b, 0x31, 0x3f, 0x63, 0x6d, 0x52, 0x5e,
    0x00, 0x74, 0x7c, 0x41, 0x4f, 0x10, 0x20, 0x62, 0x6e, 0x30, 0x73, 0x7d, 0x51, 0x5f, 0x40, 0x72, 0x7e, 0x61, 0x6f, 0x50, 0x71, 0x7f, 0x60, 0x70};
constexpr uint8_t kLengthOrder[19] = {17, 18, 0, 1, 2, 3, 4, 5, 16, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15};

struct Decoder {
  Bits br;
  const char* error = nullptr;
  Decoder(const uint8_t* d, size_t n) : br(d, n) {}
  bool fail(const char* why) { if (!error) error = why; return false; }

  bool read_code(int alphabet, Code& code, bool want_fast) {
    // (the simple form names symbols 0 .. 255 whatever the alphabet; the distance alphabet has 40, and libwebp builds from
    // the alphabet's lengths alone: a symbol beyond it is not in the code)
    std::vector<uint8_t> len((size_t)(alphabet < 256 ? 256 : alphabet), 0);
    if (br.read(1)) {  // simple
      const int two = (int)br.read(1);
      const int s0 = (int)br.read(br.read(1) ? 8 : 1);
      len[(size_t)s0] = 1;
      if (two) len[(size_t)br.read(8)] = 1;
    } else {
      uint8_t cl[19] = {};
      const int ncodes = (int)br.read(4) + 4;
      for (int i = 0; i < ncodes; ++i) cl[kLengthOrder[i]] = (uint8_t)br.read(3);
      Code lengths;
      if (!lengths.build(cl, 19, true)) return fail("vp8l: the code-length code is not a prefix code");
      int max_symbol = alphabet;
      if (br.read(1)) {
        const int nbits = 2 + 2 * (int)br.read(3);
        max_symbol = 2 + (int)br.read(nbits);
        if (max_symbol > alphabet) return fail("vp8l: max_symbol beyond the alphabet");
      }
      int s = 0, prev = 8;
      while (s < alphabet && max_symbol-- > 0) {
        if (br.eos) return fail("vp8l: the data ends inside a prefix code");
        const int c = lengths.read(br);
        if (c < 16) {
          len[(size_t)s++] = (uint8_t)c;
          if (c) prev = c;
        } else {
          const int extra = c == 16 ? 2 : c == 17 ? 3 : 7, base = c == 18 ? 11 : 3;
          const int repeat = (int)br.read(extra) + base;
          if (s + repeat > alphabet) return fail("vp8l: a code-length repeat runs beyond the alphabet");
          memset(len.data() + s, c == 16 ? prev : 0, (size_t)repeat);
          s += repeat;
        }
      }
    }
    if (br.eos) return fail("vp8l: the data ends inside a prefix code");
    if (!code.build(len.data(), alphabet, want_fast)) return fail("vp8l: a prefix code is empty, over-subscribed or incomplete");
    return true;
  }
  uint32_t prefix_value(int symbol) {  // length and distance symbols alike
    if (symbol < 4) return (uint32_t)symbol + 1;
    const int extra = (symbol - 2) >> 1;
    const uint32_t offset = (uint32_t)(2 + (symbol & 1)) << extra;
    return offset + br.read(extra) + 1;
  }

  // one entropy-coded image of xs x ys pixels; top: the main image, which alone may have a meta prefix image
  bool image(int xs, int ys, bool top, std::vector<uint32_t>& out) {
    int cache_bits = 0;
    if (br.read(1)) {
      cache_bits = (int)br.read(4);
      if (cache_bits < 1 || cache_bits > 11) return fail("vp8l: colour cache bits must be 1 .. 11");
    }
    int meta_bits = 0, meta_w = 0, ngroups = 1;
    std::vector<uint32_t> meta;
    if (top && br.read(1)) {
      meta_bits = (int)br.read(3) + 2;
      meta_w = ceil_shift(xs, meta_bits);
      if (!image(meta_w, ceil_shift(ys, meta_bits), false, meta)) return false;
      for (uint32_t& v : meta) { v = (v >> 8) & 0xFFFF; if ((int)v + 1 > ngroups) ngroups = (int)v + 1; }
    }
    if (br.eos) return fail("vp8l: the data ends inside an image header");
    std::vector<Code> codes((size_t)ngroups * 5);
    const int green = 256 + 24 + (cache_bits ? 1 << cache_bits : 0);
    for (int g = 0; g < ngroups; ++g)
      for (int j = 0; j < 5; ++j)
        if (!read_code(j == 0 ? green : j == 4 ? 40 : 256, codes[(size_t)g * 5 + j], ngroups <= 256)) return false;
    std::vector<uint32_t> cache(cache_bits ? (size_t)1 << cache_bits : 0);
    const int shift = 32 - cache_bits;
    const size_t total = (size_t)xs * ys;
    out.assign(total, 0);
    size_t pos = 0;
    const Code* g = codes.data();
    size_t col = 0, row = 0;  // of pos
    while (pos < total) {
      if (br.eos) return fail("vp8l: the data ends inside the pixels");
      if (meta_bits) g = codes.data() + 5 * (size_t)meta[(row >> meta_bits) * meta_w + (col >> meta_bits)];
      const int s = g[0].read(br);
      if (s < 256) {
        const uint32_t r = (uint32_t)g[1].read(br), b = (uint32_t)g[2].read(br), a = (uint32_t)g[3].read(br);
        const uint32_t v = (a << 24) | (r << 16) | ((uint32_t)s << 8) | b;
        out[pos++] = v;
        if (cache_bits) cache[(v * 0x1e35a7bdu) >> shift] = v;
        if (++col == (size_t)xs) { col = 0; ++row; }
      } else if (s < 280) {
        const size_t length = prefix_value(s - 256);
        const uint32_t dcode = prefix_value(g[4].read(br));
        size_t dist;
        if (dcode > 120) dist = dcode - 120;
        else {
          const int e = kShort[dcode - 1];
          const long d = (long)(e >> 4) * xs + (8 - (e & 15));
          dist = d >= 1 ? (size_t)d : 1;
        }
        if (br.eos) return fail("vp8l: the data ends inside the pixels");
        if (dist > pos) return fail("vp8l: a back reference starts before the image");
        if (length > total - pos) return fail("vp8l: a back reference runs past the image");
        for (size_t k = 0; k < length; ++k, ++pos) {
          const uint32_t v = out[pos - dist];
          out[pos] = v;
          if (cache_bits) cache[(v * 0x1e35a7bdu) >> shift] = v;
        }
        col += length;
        row += col / (size_t)xs;
        col %= (size_t)xs;
      } else {
        const size_t key = (size_t)s - 280;
        if (key >= cache.size()) return fail("vp8l: a colour-cache symbol without a cache");
        out[pos++] = cache[key];
        if (++col == (size_t)xs) { col = 0; ++row; }
      }
    }
    if (br.eos) return fail("vp8l: the data ends inside the pixels");
    return true;
  }
};

inline uint32_t le32(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }

}  // namespace detail

inline bool is_webp(const uint8_t* d, size_t n) { return n >= 12 && !memcmp(d, "RIFF", 4) && !memcmp(d + 8, "WEBP", 4); }

// the VP8L chunk's payload -> frame
inline bool parse_vp8l(const uint8_t* d, size_t n, Frame& f) {
  auto fail = [&](const char* why) { f.error = why; return false; };
  if (n < 5 || d[0] != 0x2f) return fail("vp8l: no signature");
  detail::Decoder dec(d + 1, n - 1);
  detail::Bits& br = dec.br;
  f.width = (int)br.read(14) + 1;
  f.height = (int)br.read(14) + 1;
  br.read(1);  // alpha_is_used: a hint, ignored
  if (br.read(3) != 0) return fail("vp8l: version is not 0");
  if ((long)f.width * f.height > kMaxPixels) return fail("webp: more than 64 Mpixel");
  f.transforms.clear();
  unsigned seen = 0;
  int w = f.width;
  while (br.read(1)) {
    Transform tr;
    tr.kind = (int)br.read(2);
    if (seen & (1u << tr.kind)) return fail("vp8l: a transform occurs twice");
    seen |= 1u << tr.kind;
    if (tr.kind == PREDICTOR || tr.kind == CROSS_COLOUR) {
      tr.bits = (int)br.read(3) + 2;
      if (!dec.image(ceil_shift(w, tr.bits), ceil_shift(f.height, tr.bits), false, tr.data)) return fail(dec.error);
    } else if (tr.kind == COLOUR_INDEXING) {
      const int colours = (int)br.read(8) + 1;
      tr.bits = index_bits((size_t)colours);
      if (!dec.image(colours, 1, false, tr.data)) return fail(dec.error);
      for (int i = 1; i < colours; ++i) {  // delta-coded, byte by byte
        const uint32_t a = tr.data[(size_t)i], b = tr.data[(size_t)i - 1];
        tr.data[(size_t)i] = (((a & 0xFF00FF00u) + (b & 0xFF00FF00u)) & 0xFF00FF00u) | (((a & 0x00FF00FFu) + (b & 0x00FF00FFu)) & 0x00FF00FFu);
      }
      w = ceil_shift(w, tr.bits);
    }
    f.transforms.push_back(std::move(tr));
    if (br.eos) return fail("vp8l: the data ends inside the transforms");
  }
  if (br.eos) return fail("vp8l: the data ends inside the header");
  if (!dec.image(w, f.height, true, f.argb)) return fail(dec.error);
  f.device_ok = device_scope(f);
  return true;
}

// a whole file -> frame; false: refused, f.error says why (kNotLossless for lossy and animated files)
inline bool parse(const uint8_t* d, size_t n, Frame& f) {
  auto fail = [&](const char* why) { f.error = why; return false; };
  f = Frame();
  if (!is_webp(d, n)) return fail("webp: not a RIFF / WEBP file");
  const size_t riff = detail::le32(d + 4);
  if (riff < 12 || riff > n - 8) return fail("webp: the RIFF size is beyond the file");
  n = riff + 8;  // what follows the RIFF chunk is not the file's
  size_t pos = 12;
  bool vp8x = false, first = true, alph = false;
  int canvas_w = 0, canvas_h = 0;
  while (pos + 8 <= n) {
    const uint8_t* tag = d + pos;
    const size_t size = detail::le32(d + pos + 4);
    if (size > n - pos - 8) return fail("webp: a chunk size is beyond the file");
    const uint8_t* body = d + pos + 8;
    if (!memcmp(tag, "VP8X", 4) && first) {
      if (size < 10) return fail("webp: a short VP8X chunk");
      if (body[0] & 0x02) return fail(kNotLossless);
      canvas_w = 1 + (body[4] | (body[5] << 8) | (body[6] << 16));
      canvas_h = 1 + (body[7] | (body[8] << 8) | (body[9] << 16));
      vp8x = true;
    } else if (!memcmp(tag, "ANIM", 4) || !memcmp(tag, "ANMF", 4)) {
      return fail(kNotLossless);
    } else if (!memcmp(tag, "VP8 ", 4)) {
      f.vp8 = body;
      f.vp8_size = size;
      if (vp8x) { f.canvas_width = canvas_w; f.canvas_height = canvas_h; }
      return fail(kNotLossless);
    } else if (!memcmp(tag, "ALPH", 4)) {
      if (!vp8x) return fail(kNotLossless);
      alph = true;
    } else if (!memcmp(tag, "VP8L", 4)) {
      if (alph) return fail(kNotLossless);
      if (!parse_vp8l(body, size, f)) return false;
      if (vp8x && (canvas_w != f.width || canvas_h != f.height)) return fail("webp: the VP8X canvas is not the image's size");
      return true;
    } else if (!vp8x) {
      return fail("webp: neither a VP8L nor a VP8X chunk in front");
    }
    first = false;
    pos += 8 + size + (size & 1);
  }
  return fail(alph ? kNotLossless : "webp: no image chunk");
}

// ----------------------------------------------------------------------------------------------------------- the pixel half
namespace detail {

inline uint32_t add_bytes(uint32_t a, uint32_t b) {
  return (((a & 0xFF00FF00u) + (b & 0xFF00FF00u)) & 0xFF00FF00u) | (((a & 0x00FF00FFu) + (b & 0x00FF00FFu)) & 0x00FF00FFu);
}
inline uint32_t avg2(uint32_t a, uint32_t b) { return (a & b) + (((a ^ b) & 0xFEFEFEFEu) >> 1); }
inline int clamp255(int v) { return v < 0 ? 0 : v > 255 ? 255 : v; }
inline uint32_t select(uint32_t L, uint32_t T, uint32_t TL) {
  int pl = 0, pt = 0;  // distance of the estimate L + T - TL to L and to T
  for (int s = 0; s < 32; s += 8) {
    pl += abs((int)((T >> s) & 255) - (int)((TL >> s) & 255));
    pt += abs((int)((L >> s) & 255) - (int)((TL >> s) & 255));
  }
  return pt <= pl ? T : L;
}
inline uint32_t clamp_full(uint32_t L, uint32_t T, uint32_t TL) {
  uint32_t r = 0;
  for (int s = 0; s < 32; s += 8) r |= (uint32_t)clamp255((int)((L >> s) & 255) + (int)((T >> s) & 255) - (int)((TL >> s) & 255)) << s;
  return r;
}
inline uint32_t clamp_half(uint32_t L, uint32_t T, uint32_t TL) {
  const uint32_t a = avg2(L, T);
  uint32_t r = 0;
  for (int s = 0; s < 32; s += 8) {
    const int x = (int)((a >> s) & 255), y = (int)((TL >> s) & 255);
    r |= (uint32_t)clamp255(x + (x - y) / 2) << s;
  }
  return r;
}
template <int M> inline uint32_t predict(uint32_t L, uint32_t T, uint32_t TL, uint32_t TR) {
  switch (M) {
    case 1: return L;
    case 2: return T;
    case 3: return TR;
    case 4: return TL;
    case 5: return avg2(avg2(L, TR), T);
    case 6: return avg2(L, TL);
    case 7: return avg2(L, T);
    case 8: return avg2(TL, T);
    case 9: return avg2(T, TR);
    case 10: return avg2(avg2(L, TL), avg2(T, TR));
    case 11: return select(L, T, TL);
    case 12: return clamp_full(L, T, TL);
    case 13: return clamp_half(L, T, TL);
    default: return 0xFF000000u;
  }
}
// pixels [x0, x1) of a row (x0 >= 1, a row above exists): cur[x] += predict(...)
template <int M> inline void predict_span(uint32_t* cur, const uint32_t* up, int x0, int x1) {
  for (int x = x0; x < x1; ++x) cur[x] = add_bytes(cur[x], predict<M>(cur[x - 1], up[x], up[x - 1], up[x + 1]));
}
inline void predict_mode(int m, uint32_t* cur, const uint32_t* up, int x0, int x1) {
  switch (m) {
#define WEBP_MODE(M) case M: predict_span<M>(cur, up, x0, x1); break;
    WEBP_MODE(1) WEBP_MODE(2) WEBP_MODE(3) WEBP_MODE(4) WEBP_MODE(5) WEBP_MODE(6) WEBP_MODE(7) WEBP_MODE(8) WEBP_MODE(9) WEBP_MODE(10)
    WEBP_MODE(11) WEBP_MODE(12) WEBP_MODE(13)
#undef WEBP_MODE
    default: predict_span<0>(cur, up, x0, x1); break;
  }
}
inline void undo_predictor(uint32_t* px, int w, int h, const Transform& tr) {
  const int bw = ceil_shift(w, tr.bits), bs = 1 << tr.bits;
  px[0] = add_bytes(px[0], 0xFF000000u);
  for (int x = 1; x < w; ++x) px[x] = add_bytes(px[x], px[x - 1]);
  for (int y = 1; y < h; ++y) {
    uint32_t* cur = px + (size_t)y * w;
    const uint32_t* up = cur - w;  // (up[w] is cur[0]: TR of the last column)
    cur[0] = add_bytes(cur[0], up[0]);
    const uint32_t* modes = tr.data.data() + (size_t)(y >> tr.bits) * bw;
    for (int x0 = 0; x0 < w; x0 += bs) predict_mode((int)(modes[x0 >> tr.bits] >> 8) & 15, cur, up, x0 ? x0 : 1, x0 + bs < w ? x0 + bs : w);
  }
}
inline uint32_t cross_colour(uint32_t v, uint32_t m) {
  const int g2r = (int8_t)(m & 255), g2b = (int8_t)((m >> 8) & 255), r2b = (int8_t)((m >> 16) & 255);
  const int green = (int8_t)((v >> 8) & 255);
  const uint32_t red = ((v >> 16) + (uint32_t)((g2r * green) >> 5)) & 255;
  uint32_t blue = v + (uint32_t)((g2b * green) >> 5);
  blue = (blue + (uint32_t)((r2b * (int)(int8_t)red) >> 5)) & 255;
  return (v & 0xFF00FF00u) | (red << 16) | blue;
}
inline uint32_t add_green(uint32_t v) {
  const uint32_t g = (v >> 8) & 255;
  return (v & 0xFF00FF00u) | (((v & 0x00FF00FFu) + (g << 16 | g)) & 0x00FF00FFu);
}

}  // namespace detail

// the exact-parity host stage: frame -> packed BGR, height x width (alpha dropped); false when fault(frame)
inline bool pixels(const Frame& f, std::vector<uint8_t>& bgr) {
  if (fault(f)) return false;
  const int h = f.height;
  int w = coded_width(f);
  std::vector<uint32_t> px(f.argb.begin(), f.argb.begin() + (size_t)w * h), wide;
  for (size_t t = f.transforms.size(); t-- > 0;) {
    const Transform& tr = f.transforms[t];
    switch (tr.kind) {
      case PREDICTOR: detail::undo_predictor(px.data(), w, h, tr); break;
      case CROSS_COLOUR: {
        const int bw = ceil_shift(w, tr.bits);
        for (int y = 0; y < h; ++y) {
          uint32_t* row = px.data() + (size_t)y * w;
          const uint32_t* m = tr.data.data() + (size_t)(y >> tr.bits) * bw;
          for (int x = 0; x < w; ++x) row[x] = detail::cross_colour(row[x], m[x >> tr.bits]);
        }
        break;
      }
      case ADD_GREEN:
        for (uint32_t& v : px) v = detail::add_green(v);
        break;
      default: {  // colour indexing: w coded pixels a row -> the width in front of it
        const int full = width_at(f, t), per = 1 << tr.bits, each = 8 >> tr.bits;
        uint32_t pal[256] = {};
        memcpy(pal, tr.data.data(), tr.data.size() * 4);
        wide.resize((size_t)full * h);
        for (int y = 0; y < h; ++y)
          for (int x = 0; x < full; ++x) {
            const uint32_t packed = (px[(size_t)y * w + (x >> tr.bits)] >> 8) & 255;
            wide[(size_t)y * full + x] = pal[(packed >> ((x & (per - 1)) * each)) & ((1u << each) - 1)];
          }
        px.swap(wide);
        w = full;
        break;
      }
    }
  }
  bgr.resize((size_t)w * h * 3);
  for (size_t i = 0; i < (size_t)w * h; ++i) {
    bgr[3 * i] = (uint8_t)px[i];
    bgr[3 * i + 1] = (uint8_t)(px[i] >> 8);
    bgr[3 * i + 2] = (uint8_t)(px[i] >> 16);
  }
  return true;
}

}  // namespace webp
}  // namespace PaddleOCR
