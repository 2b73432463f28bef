// TIFF decoder in two halves, shaped like png_decode.h / raw_decode.h: the container and whatever is serial (the IFD, the
// chunk tables, PackBits / LZW / Deflate expansion, FillOrder) on the caller's host thread - parse() - and the pixel part
// (the horizontal-differencing predictor, tile placement, planar to chunky, bit expansion, palette, MinIsWhite, 16 -> 8 bits,
// CMYK, alpha) either on the device (csrc/kernels_tiff.hip, through ocr_tiff_frame) or here - pixels().
//
// What comes out is what cv::imdecode(data, IMREAD_COLOR) returns, on the understanding (from memory of OpenCV 4.x's
// grfmt_tiff.cpp: UNPINNED) that its 8-bit path reads through libtiff's RGBA interface
// (TIFFReadRGBAStrip / TIFFReadRGBATile), drops alpha and swaps to BGR.  The rules of that interface below ARE pinned:
// tests/test_tiff_decode.py compares every form with TIFFReadRGBAImageOriented of the system's libtiff (4.3.0).
//
// Container: classic TIFF, "II*\0" or "MM\0*" (BigTIFF, magic 43, is refused), the first IFD only.  Tag values inline or at
// an offset, of type BYTE, SHORT or LONG (a tag this decoder reads with another type refuses the file; tags it does not
// read are skipped whatever they are).  Every offset and count is checked against the bytes present before anything is
// allocated; width * height <= 64 Mpixel; the chunk tables must lie in the file, which bounds the number of chunks.
//   - ImageWidth, ImageLength, PhotometricInterpretation and the chunk offsets and byte counts are required
//   - strips: any RowsPerStrip (absent, or above the height: one strip); tiles: TileWidth and TileLength multiples of 16
//   - PlanarConfiguration 1; 2 for RGB(A) and for grey with extra samples, 8 and 16 bits
//   - Compression 1, 32773 (PackBits), 5 (LZW, MSB first with the early width change; the old LSB-first variant - a stream
//     that begins 00 and an odd byte - is refused), 8 and 32946 (Deflate, through the zlib png_decode.h resolved).  A chunk
//     that expands to fewer bytes than its geometry needs refuses the file; surplus is ignored.  An LZW code beyond the
//     table refuses the file.  FillOrder 2 reverses the bits of every coded byte first
//   - BitsPerSample the same for every sample; SampleFormat absent or 1; Predictor 1, or 2 with LZW / Deflate at 8 and
//     16 bits (libtiff takes the tag from those codecs alone: with Compression 1 or PackBits it is not read, here neither)
// Samples (libtiff's tif_getimage.c):
//   - grey (photometric 0 / 1), chunky: 1, 2, 4 bits v * 255 / (2^bits - 1); 8 bits v; 16 bits the HIGH byte; MinIsWhite
//     255 - that.  Extra samples (8 / 16 bits) are skipped, whatever ExtraSamples calls them: nothing premultiplies
//   - grey with extra samples in planes (planar 2) goes the way of RGB: 16 bits (v + 128) / 257, unassociated alpha
//     premultiplies, and MinIsWhite is NOT inverted
//   - palette 1, 2, 4, 8 bits: ColorMap holds 16-bit values, reduced by >> 8 - unless no entry of the first 2^bits of each
//     colour is 256 or more: then the map is taken for an 8-bit one and used as it is
//   - RGB 8 bits as stored; 16 bits (v + 128) / 257.  ExtraSamples[0] = 2 (unassociated alpha): c = (c * a + 127) / 255
//     with the reduced a; 1 (associated) and 0 (unspecified): the colour as stored.  Alpha is then dropped
//   - CMYK 8 bits chunky: (255 - c) * (255 - k) / 255, rounded down; InkSet absent or 1; samples beyond the four skipped
//   - 16-bit words are read in the file's byte order, and the predictor's sum runs on those words
//   - Compression 2, 32771 (Modified Huffman RLE), 3 (T.4 / Group 3, 1-D and 2-D) and 4 (T.6 / Group 4): bilevel fax pages,
//     through ccitt_decode.h, which states what is decoded.  1 bit, 1 sample, photometric 0 or 1, no predictor; T4Options
//     absent means 0.  The chunks come out as 1-bit rows, white 0 and black 1 whatever the photometric says, and go the way of
//     1-bit grey.  A damaged stream refuses the file with a reason (fax_why) - stricter than libtiff, which patches such rows
//     with white and warns, as for LZW above; uncompressed mode (T4Options / T6Options bit 1) is refused, as libtiff does
// Orientation is ignored: rows are taken as stored (UNPINNED).  YCbCr, CIELab, masks and JPEG compression
// are refused.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

#include "ccitt_decode.h"
#include "png_decode.h"

namespace PaddleOCR {
namespace tiff {

constexpr long kMaxPixels = 64L << 20;          // the cap of the service's other decoders (kMaxDecodedPixels)
constexpr size_t kMaxBytes = (size_t)1 << 30;   // of the expanded chunks at their nominal size (64 Mpixel RGBA at 16 bits: half of it)
constexpr int kMaxSamples = 16;                 // per pixel
// What the device pixel stage takes; a frame beyond is finished on the host.  The stage keeps no table per chunk or row - a
// unit of its work is found by division - so the bound is on what a header can make it walk: chunks at their nominal size.
constexpr size_t kMaxDeviceChunks = 1u << 20;
constexpr size_t kMaxDeviceBytes = (size_t)1 << 29;
constexpr int kMaxFaxDeviceWidth = 8192;  // pixels of a CCITT chunk row that the device expansion takes (csrc/kernels_tiff_fax.h)

struct Frame {  // ocr_tiff_frame of include/ocr_hip.h, field for field
  int width = 0, height = 0;
  int photometric = 1;   // 0 MinIsWhite, 1 MinIsBlack, 2 RGB, 3 palette, 5 CMYK
  int bits = 1;          // per sample: 1, 2, 4, 8, 16
  int samples = 1;       // per pixel as stored, extra samples included
  int planar = 1;        // 1: samples of a pixel side by side; 2: one plane of chunks per sample
  int predictor = 1;     // 2: every sample is stored as the difference from the sample of the pixel before it in the chunk's row
  int big_endian = 0;    // of 16-bit samples
  int premultiply = 0;   // 1: the sample behind the colour samples is unassociated alpha and multiplies them
  int tile_width = 0, tile_height = 0;  // a chunk; a strip is a chunk as wide as the image, RowsPerStrip (at most the height) high
  uint8_t palette[1024] = {};           // B,G,R,x times 256, reduced to 8 bits
  // the expanded chunks, each at its nominal size tile_height * row bytes, chunk (cy, cx) of plane p at
  // ((p * chunks down + cy) * chunks across + cx) * that size; rows of a strip the image does not have are zero
  std::vector<uint8_t> data;
  bool device_ok = false;  // within kMaxDeviceChunks / kMaxDeviceBytes: the device pixel stage may take the frame
};

struct Geometry {
  int across = 0, down = 0, planes = 1;  // chunks, and planes of them
  int colour = 1;                        // colour samples: 1, 3 or 4
  int used = 1;                          // the leading samples a pixel is made of (colour, and alpha when it premultiplies)
  size_t row_bytes = 0, chunk_bytes = 0, total = 0;
};

// The rules a frame satisfies (csrc/capi_tiff.hip checks the same on its side of the ABI); nullptr when it is sound.
inline const char* fault(const Frame& f, Geometry& g) {
  if (f.width <= 0 || f.height <= 0 || (long)f.width * f.height > kMaxPixels) return "width and height must be positive and at most 64 Mpixel together";
  if (f.bits != 1 && f.bits != 2 && f.bits != 4 && f.bits != 8 && f.bits != 16) return "bits per sample must be 1, 2, 4, 8 or 16";
  if (f.samples < 1 || f.samples > kMaxSamples) return "samples per pixel must be 1 .. 16";
  if (f.planar != 1 && f.planar != 2) return "planar must be 1 or 2";
  if (f.predictor != 1 && f.predictor != 2) return "predictor must be 1 or 2";
  if ((f.big_endian | 1) != 1 || (f.premultiply | 1) != 1) return "big_endian and premultiply must be 0 or 1";
  const int ph = f.photometric;
  if (ph != 0 && ph != 1 && ph != 2 && ph != 3 && ph != 5) return "photometric must be 0, 1, 2, 3 or 5";
  g.colour = ph == 2 ? 3 : ph == 5 ? 4 : 1;
  if (f.samples < g.colour) return "fewer samples per pixel than the photometric needs";
  if (f.bits < 8 && (ph == 2 || ph == 5 || f.samples != 1 || f.predictor != 1 || f.planar != 1)) return "1, 2 and 4 bits: grey or palette, one sample, no predictor, chunky";
  if (ph == 3 && (f.bits > 8 || f.planar != 1)) return "palette: at most 8 bits, chunky";
  if (ph == 5 && (f.bits != 8 || f.planar != 1)) return "CMYK: 8 bits, chunky";
  if (f.planar == 2 && ph != 2 && f.samples < 2) return "planar 2: RGB, or grey with extra samples";
  if (f.premultiply && (f.samples <= g.colour || !(ph == 2 || (ph <= 1 && f.planar == 2)))) return "premultiply: RGB with alpha, or grey with alpha in planes";
  if (f.tile_width <= 0 || f.tile_height <= 0 || (long)f.tile_width * f.tile_height > kMaxPixels) return "tile_width and tile_height must be positive and at most 64 Mpixel together";
  g.used = g.colour + f.premultiply;
  g.planes = f.planar == 2 ? f.samples : 1;
  g.across = (int)(((long)f.width + f.tile_width - 1) / f.tile_width);
  g.down = (int)(((long)f.height + f.tile_height - 1) / f.tile_height);
  g.row_bytes = ((size_t)f.tile_width * (f.planar == 2 ? 1 : f.samples) * f.bits + 7) / 8;  // <= 2^26 * 32
  g.chunk_bytes = g.row_bytes * (size_t)f.tile_height;                                      // <= 2^26 * 32 + 2^26
  g.total = g.chunk_bytes * (size_t)g.across * g.down * g.planes;                           // < 2^32 * 2^26 * 2^4
  if (g.total > kMaxBytes) return "the chunks at their nominal size exceed 1 GiB";
  return nullptr;
}
inline bool sound(const Frame& f, Geometry& g) { return !fault(f, g) && f.data.size() >= g.total; }

// A file before its chunks are expanded (Compression 1, 5 and 32773): parse() is parse_coded() + expand(), and the device
// takes the second half too (csrc/kernels_tiff_lzw.hip through ocr_tiff_coded).  A Deflate file (8, 32946) has the same form
// from parse_deflate(), whose second half is inflate_all() here and csrc/kernels_inflate.hip on the device.
struct Chunk {  // ocr_tiff_chunk of include/ocr_hip.h, field for field
  uint64_t byte_off = 0;  // into Coded::bytes
  uint32_t byte_len = 0;
  uint32_t rows = 0;      // the rows the chunk really holds: 1 .. tile_height (the last strip may have fewer)
};
struct Coded {
  Frame frame;                // data empty
  int compression = 1;        // 1, 5 (LZW) or 32773 (PackBits); 8 or 32946 (Deflate) from parse_deflate alone
  std::vector<Chunk> chunks;  // in the order Frame::data has them: plane by plane, row of chunks by row of chunks
  std::vector<uint8_t> bytes; // the coded chunks one after another, MSB first (FillOrder 2 is undone)
  uint32_t t4_options = 0;    // a fax frame (compression 2, 3, 4 or 32771, from parse_fax alone): T4Options of Compression 3, else 0
};
// of parse_coded; kOtherRoute: Deflate, which goes through parse(); kFaxRoute: a sound CCITT file, which parse_fax() hands over
enum Route { kRefused = 0, kCoded = 1, kOtherRoute = 2, kFaxRoute = 3 };

namespace detail {

struct Reader {  // the file, in its byte order
  const uint8_t* d; size_t n; bool be;
  uint32_t u16(size_t o) const { return be ? ((uint32_t)d[o] << 8) | d[o + 1] : (uint32_t)d[o] | ((uint32_t)d[o + 1] << 8); }
  uint32_t u32(size_t o) const { return be ? (u16(o) << 16) | u16(o + 2) : u16(o) | (u16(o + 2) << 16); }
};
struct Tag {  // an IFD entry of type BYTE, SHORT or LONG whose values lie in the file
  bool present = false;
  uint32_t type = 0, count = 0;
  size_t at = 0;  // of the first value
};
inline uint32_t value(const Reader& r, const Tag& t, size_t i) { return t.type == 1 ? r.d[t.at + i] : t.type == 3 ? r.u16(t.at + 2 * i) : r.u32(t.at + 4 * i); }

inline uint8_t reverse_bits(uint8_t b) { b = (uint8_t)((b >> 4) | (b << 4)); b = (uint8_t)(((b & 0xCC) >> 2) | ((b & 0x33) << 2)); return (uint8_t)(((b & 0xAA) >> 1) | ((b & 0x55) << 1)); }

// The expanders write `need` bytes at out (room for exactly that many) and say whether the stream had them.
inline bool unpack_bits(const uint8_t* s, size_t n, uint8_t* out, size_t need) {
  size_t i = 0, o = 0;
  while (o < need && i < n) {
    const int c = (int8_t)s[i++];
    if (c >= 0) {  // c + 1 literal bytes
      size_t k = (size_t)c + 1;
      if (n - i < k) k = n - i;
      if (k > need - o) k = need - o;
      memcpy(out + o, s + i, k);
      i += (size_t)c + 1; o += k;
      if (i > n) break;
    } else if (c != -128) {  // the next byte 1 - c times
      if (i >= n) break;
      size_t k = (size_t)(1 - c);
      if (k > need - o) k = need - o;
      memset(out + o, s[i++], k);
      o += k;
    }
  }
  return o == need;
}

inline bool unlzw(const uint8_t* s, size_t n, uint8_t* out, size_t need) {
  if (need == 0) return true;
  if (n >= 2 && s[0] == 0 && (s[1] & 1)) return false;  // the old LSB-first variant (libtiff's test for it)
  struct Entry { uint16_t prev; uint16_t len; uint8_t first, last; };  // a string = the string of prev + last
  std::vector<Entry> tab(4096);
  for (int i = 0; i < 256; ++i) tab[i] = Entry{0, 1, (uint8_t)i, (uint8_t)i};
  int bits = 9, next = 258, old = -1;
  uint64_t acc = 0;
  int have = 0;
  size_t i = 0, o = 0;
  while (o < need) {
    while (have < bits && i < n) { acc = (acc << 8) | s[i++]; have += 8; }
    if (have < bits) break;  // the stream ends
    const int code = (int)((acc >> (have - bits)) & ((1u << bits) - 1));
    have -= bits;
    if (code == 256) { bits = 9; next = 258; old = -1; continue; }
    if (code == 257) break;
    if (old < 0) {  // the first code behind a clear is a byte
      if (code > 255) return false;
      out[o++] = (uint8_t)code;
      old = code;
      continue;
    }
    if (code > next || next >= 4096) return false;  // a code beyond the table, or a table that was never cleared
    tab[next] = Entry{(uint16_t)old, (uint16_t)(tab[old].len + 1), tab[old].first, code < next ? tab[code].first : tab[old].first};
    ++next;
    if (next > (1 << bits) - 2 && bits < 12) ++bits;  // the early change: 511, 1023 and 2047 entries
    // the string of `code`, written from its end (what does not fit is dropped)
    const size_t len = tab[code].len, take = len < need - o ? len : need - o;
    int c = code;
    for (size_t k = len; k > 0; --k, c = tab[c].prev)
      if (k <= take) out[o + k - 1] = tab[c].last;
    o += take;
    old = code;
  }
  return o == need;
}

// The extent scans: the walks of unpack_bits and unlzw over the lengths alone - no byte is copied, no chain is followed.
// They say true exactly where the expander says true for the same `need`, and stop where it stops: what lies behind the
// code that completes `need` is not looked at.  A chunk that passed is what the device expander is given.
inline bool packbits_extent(const uint8_t* s, size_t n, size_t need) {
  size_t i = 0, o = 0;
  while (o < need && i < n) {
    const int c = (int8_t)s[i++];
    if (c >= 0) {
      size_t k = (size_t)c + 1;
      if (n - i < k) k = n - i;
      if (k > need - o) k = need - o;
      i += (size_t)c + 1; o += k;
      if (i > n) break;
    } else if (c != -128) {
      if (i >= n) break;
      ++i;
      const size_t k = (size_t)(1 - c);
      o += k > need - o ? need - o : k;
    }
  }
  return o == need;
}

inline bool lzw_extent(const uint8_t* s, size_t n, size_t need) {
  if (need == 0) return true;
  if (n >= 2 && s[0] == 0 && (s[1] & 1)) return false;
  uint16_t len[4096];  // of an entry's string; an entry below `next` alone is read
  for (int i = 0; i < 258; ++i) len[i] = 1;
  int bits = 9, next = 258, old = -1;
  uint64_t acc = 0;
  int have = 0;
  size_t i = 0, o = 0;
  while (o < need) {
    while (have < bits && i < n) { acc = (acc << 8) | s[i++]; have += 8; }
    if (have < bits) break;
    const int code = (int)((acc >> (have - bits)) & ((1u << bits) - 1));
    have -= bits;
    if (code == 256) { bits = 9; next = 258; old = -1; continue; }
    if (code == 257) break;
    if (old < 0) {
      if (code > 255) return false;
      ++o;
      old = code;
      continue;
    }
    if (code > next || next >= 4096) return false;
    len[next] = (uint16_t)(len[old] + 1);
    ++next;
    if (next > (1 << bits) - 2 && bits < 12) ++bits;
    o += len[code] < need - o ? len[code] : need - o;
    old = code;
  }
  return o == need;
}

// the bytes zlib gives before its first error, the end of the stream or the end of the input, at most `need`
inline size_t inflate_count(const uint8_t* s, size_t n, uint8_t* out, size_t need) {
  const png::Zlib& z = png::zlib();
  if (!z.ok() || n > 0xFFFFFFFFu) return 0;
  png::ZStream zs;
  memset(&zs, 0, sizeof zs);
  if (z.init(&zs, "1.2.11", (int)sizeof zs) != 0) return 0;
  zs.next_in = s; zs.avail_in = (unsigned)n;
  size_t o = 0;
  bool ok = true;
  while (o < need && ok) {
    const size_t room = need - o;
    zs.next_out = out + o;
    zs.avail_out = (unsigned)(room < 0x40000000u ? room : 0x40000000u);
    const unsigned before = zs.avail_out;
    const int rc = z.inflate(&zs, 0 /* Z_NO_FLUSH */);
    o += before - zs.avail_out;
    if (rc == 1 /* Z_STREAM_END */) break;
    if (rc != 0 || before == zs.avail_out) ok = false;  // an error, or no progress (the input is used up)
  }
  z.end(&zs);
  return o;
}
// a chunk is good where `need` bytes come out; neither a wrong checksum nor a missing trailer behind them refuses it
inline bool inflate(const uint8_t* s, size_t n, uint8_t* out, size_t need) { return inflate_count(s, n, out, need) == need; }

}  // namespace detail

namespace detail {

// What the container says beyond the frame: where the chunks lie and how they are coded.
struct Head {
  Reader r{nullptr, 0, false};
  Geometry g;
  uint32_t comp = 1, fill = 1;
  uint32_t t4 = 0;            // T4Options of a Compression 3 file
  const char* why = nullptr;  // a CCITT file that is refused for a rule of its coding: which
  bool tiled = false;
  size_t chunks = 0;
  Tag offs, counts;
  // chunk c of the file: where its bytes lie, and the rows it really holds
  size_t at(size_t c) const { return value(r, offs, c); }
  size_t len(size_t c) const { return value(r, counts, c); }
  size_t rows(const Frame& f, size_t c) const {
    const size_t cy = (c / g.across) % g.down;
    return cy + 1 == (size_t)g.down && !tiled ? (size_t)f.height - cy * f.tile_height : (size_t)f.tile_height;
  }
};

// The container up to the expansion: the IFD, the frame, the chunk tables.  false = not a TIFF file, or one that is refused.
inline bool parse_head(const uint8_t* d, size_t n, Frame& f, Head& hd) {
  if (n < 8) return false;
  const bool be = d[0] == 'M';
  if (!((d[0] == 'I' && d[1] == 'I') || (d[0] == 'M' && d[1] == 'M'))) return false;
  const Reader r{d, n, be};
  hd.r = r;
  if (r.u16(2) != 42) return false;  // (43: BigTIFF)
  const size_t ifd = r.u32(4);
  if (ifd < 8 || ifd > n - 2) return false;
  const size_t entries = r.u16(ifd);
  if ((n - ifd - 2) / 12 < entries) return false;
  enum { W, H, BPS, COMP, PHOTO, FILL, OFFS, SPP, RPS, COUNTS, PLANAR, PRED, CMAP, TW, TL, TOFFS, TCOUNTS, EXTRA, FORMAT, INK, T4OPT, T6OPT, kTags };
  static const uint16_t ids[kTags] = {256, 257, 258, 259, 262, 266, 273, 277, 278, 279, 284, 317, 320, 322, 323, 324, 325, 338, 339, 332, 292, 293};
  Tag tag[kTags];
  for (size_t e = 0; e < entries; ++e) {
    const size_t at = ifd + 2 + 12 * e;
    const uint32_t id = r.u16(at), type = r.u16(at + 2), count = r.u32(at + 4);
    int k = 0;
    while (k < kTags && ids[k] != id) ++k;
    if (k == kTags) continue;  // a tag this decoder does not read
    if (tag[k].present || (type != 1 && type != 3 && type != 4) || count == 0) return false;
    const size_t size = type == 1 ? 1 : type == 3 ? 2 : 4;
    Tag t;
    t.present = true; t.type = type; t.count = count;
    if ((size_t)count <= 4 / size) t.at = at + 8;
    else {
      t.at = r.u32(at + 8);
      if (t.at < 8 || t.at > n || (n - t.at) / size < count) return false;  // (below 8: a table laid over the header)
    }
    tag[k] = t;
  }
  auto one = [&](int k, uint32_t otherwise) { return tag[k].present ? value(r, tag[k], 0) : otherwise; };
  if (!tag[W].present || !tag[H].present || !tag[PHOTO].present) return false;
  const uint32_t w = one(W, 0), h = one(H, 0);
  if (w == 0 || h == 0 || w > 0x7fffffffu || h > 0x7fffffffu || (long)w * (long)h > kMaxPixels) return false;
  const uint32_t spp = one(SPP, 1), comp = one(COMP, 1), photo = one(PHOTO, 0), fill = one(FILL, 1), planar = one(PLANAR, 1);
  uint32_t pred = one(PRED, 1);
  if (spp < 1 || spp > (uint32_t)kMaxSamples || (fill != 1 && fill != 2) || (planar != 1 && planar != 2)) return false;
  const bool fax = ccitt::is_fax((int)comp);
  if (comp != 1 && comp != 5 && comp != 8 && comp != 32946 && comp != 32773 && !fax) return false;
  if (fax) {  // the rules of the coding that the container shows
    if (pred == 2) { hd.why = "fax: CCITT coding takes no predictor"; return false; }
    if ((tag[BPS].present && (tag[BPS].count != 1 || value(r, tag[BPS], 0) != 1)) || spp != 1) { hd.why = "fax: CCITT coding needs 1 bit per sample and 1 sample per pixel"; return false; }
    if (photo > 1) { hd.why = "fax: CCITT coding needs photometric 0 or 1"; return false; }
    if ((comp == 3 && (one(T4OPT, 0) & 2)) || (comp == 4 && (one(T6OPT, 0) & 2))) { hd.why = ccitt::kUncompressed; return false; }
    if (comp == 3 && (one(T4OPT, 0) & ~7u)) { hd.why = "fax: T4Options has bits beyond 0 .. 2"; return false; }
    hd.t4 = comp == 3 ? one(T4OPT, 0) : 0;
  }
  if (comp == 1 || comp == 32773) pred = 1;  // (the tag belongs to the LZW and Deflate codecs: libtiff does not read it here)
  if (pred != 1 && pred != 2) return false;
  uint32_t bits = 1;
  if (tag[BPS].present) {
    if (tag[BPS].count != spp && !(tag[BPS].count == 1 && spp == 1)) return false;
    bits = value(r, tag[BPS], 0);
    for (uint32_t i = 1; i < tag[BPS].count; ++i) if (value(r, tag[BPS], i) != bits) return false;
  } else if (spp != 1) return false;
  if (tag[FORMAT].present)
    for (uint32_t i = 0; i < tag[FORMAT].count; ++i) if (value(r, tag[FORMAT], i) != 1) return false;
  if (tag[INK].present && one(INK, 1) != 1) return false;
  f = Frame();
  f.width = (int)w; f.height = (int)h; f.photometric = (int)photo; f.bits = (int)bits; f.samples = (int)spp; f.planar = (int)planar;
  f.predictor = (int)pred; f.big_endian = be;
  if (photo > 5) return false;
  const int colour = photo == 2 ? 3 : photo == 5 ? 4 : 1;
  uint32_t extras = 0;
  if (tag[EXTRA].present) {
    extras = tag[EXTRA].count;
    if (extras >= spp || (int)(spp - extras) < colour) return false;
    // the first extra sample alone says whether there is alpha, and only where libtiff's RGB routines do the work
    if (value(r, tag[EXTRA], 0) == 2 && (photo == 2 || (photo <= 1 && planar == 2))) {
      if ((int)(spp - extras) != colour) return false;  // (alpha would not be the sample behind the colour)
      f.premultiply = 1;
    }
  }
  if (planar == 2 && spp == 1) f.planar = 1;  // (one plane is chunky)
  const bool tiled = tag[TW].present || tag[TL].present;
  if (tiled) {
    const uint32_t tw = one(TW, 0), tl = one(TL, 0);
    if (tw == 0 || tl == 0 || tw % 16 || tl % 16 || tw > (1u << 26) || tl > (1u << 26)) return false;
    f.tile_width = (int)tw; f.tile_height = (int)tl;
  } else {
    const uint32_t rps = one(RPS, 0xFFFFFFFFu);
    if (rps == 0) return false;
    f.tile_width = (int)w; f.tile_height = (int)(rps < h ? rps : h);
  }
  Geometry& g = hd.g;
  if (fault(f, g)) return false;
  // the chunk tables: as many entries as the geometry has chunks (they lie in the file: that bounds the number)
  const Tag& offs = tag[tiled ? TOFFS : OFFS];
  const Tag& counts = tag[tiled ? TCOUNTS : COUNTS];
  const size_t chunks = hd.chunks = (size_t)g.across * g.down * g.planes;
  if (!offs.present || !counts.present || offs.count != chunks || counts.count != chunks) return false;
  if (photo == 3) {
    const size_t entries3 = (size_t)1 << bits;
    if (!tag[CMAP].present || tag[CMAP].type != 3 || tag[CMAP].count != 3 * entries3) return false;
    bool wide = false;  // any value of 256 or more: a 16-bit map, reduced by >> 8; else it is taken for an 8-bit one
    for (size_t i = 0; i < 3 * entries3; ++i) wide = wide || value(r, tag[CMAP], i) >= 256;
    for (size_t i = 0; i < entries3; ++i)
      for (int c = 0; c < 3; ++c) {  // the map holds all reds, then all greens, then all blues
        const uint32_t v = value(r, tag[CMAP], (size_t)c * entries3 + i);
        f.palette[4 * i + 2 - c] = (uint8_t)(wide ? v >> 8 : v);
      }
  }
  // every chunk's bytes lie in the file, and an uncompressed one has what its geometry needs, before anything is allocated
  size_t coded = 0;
  for (size_t c = 0; c < chunks; ++c) {
    const size_t at = value(r, offs, c), len = value(r, counts, c);
    if (at < 8 || at > n || n - at < len) return false;
    const size_t cy = (c / g.across) % g.down;
    const size_t rows = cy + 1 == (size_t)g.down && !tiled ? (size_t)h - cy * f.tile_height : (size_t)f.tile_height;
    if (comp == 1 && len < rows * g.row_bytes) return false;
    // no codec here expands beyond 2800 to 1 (LZW: a 12-bit code for a string of 4094 bytes at most; Deflate 1032, PackBits 64)
    // a fax row takes a bit at least (a V0 code)
    if (fax ? rows / 8 > len : comp != 1 && rows * g.row_bytes / 2800 > len) return false;
    coded += len;
  }
  if (comp != 1 && coded == 0) return false;
  hd.comp = comp; hd.fill = fill; hd.tiled = tiled; hd.offs = offs; hd.counts = counts;
  return true;
}

// the chunk records of a frame whose geometry is g: as many as the geometry has chunks, each with rows the chunk can hold and
// bytes inside the pool
inline const char* records_fault(const Frame& f, const Geometry& g, const Chunk* chunks, size_t nchunks, size_t pool) {
  if (nchunks != (size_t)g.across * g.down * g.planes || (nchunks && !chunks)) return "coded: as many chunk records as the geometry has chunks";
  for (size_t c = 0; c < nchunks; ++c) {
    if (chunks[c].rows < 1 || chunks[c].rows > (uint32_t)f.tile_height) return "coded: a chunk's rows must be 1 .. tile_height";
    if (chunks[c].byte_off > pool || pool - chunks[c].byte_off < chunks[c].byte_len) return "coded: a chunk's bytes lie outside the pool";
  }
  return nullptr;
}

inline const char* structure_fault(const Frame& f, int compression, const Chunk* chunks, size_t nchunks, size_t pool, Geometry& g, bool deflate = false) {
  if (const char* why = fault(f, g)) return why;
  if (deflate) {
    if (compression != 8 && compression != 32946) return "deflate: compression must be 8 or 32946 (Deflate)";
  } else if (compression != 1 && compression != 5 && compression != 32773) return "coded: compression must be 1 (none), 5 (LZW) or 32773 (PackBits)";
  return records_fault(f, g, chunks, nchunks, pool);
}

}  // namespace detail

// The rules a coded frame satisfies, over its parts (csrc/capi_tiff.hip runs the same text on its side of the ABI): fault(),
// the records, and the extent scan of every chunk - a faulty stream is found here, on the host, because the device expander
// cannot refuse a file.  nullptr when it is sound.
inline const char* coded_fault_of(const Frame& f, int compression, const Chunk* chunks, size_t nchunks, const uint8_t* bytes, size_t pool, Geometry& g) {
  if (const char* why = detail::structure_fault(f, compression, chunks, nchunks, pool, g)) return why;
  if (pool && !bytes) return "coded: the byte pool is missing";
  for (size_t c = 0; c < nchunks; ++c) {
    const uint8_t* s = bytes + chunks[c].byte_off;
    const size_t len = chunks[c].byte_len, need = (size_t)chunks[c].rows * g.row_bytes;
    const bool ok = compression == 1 ? len >= need : compression == 5 ? detail::lzw_extent(s, len, need) : detail::packbits_extent(s, len, need);
    if (!ok) return "coded: a chunk's stream does not hold the bytes its rows need";
  }
  return nullptr;
}
inline const char* coded_fault(const Coded& c, Geometry& g) {
  if (!c.frame.data.empty()) return "coded: a coded frame carries no expanded chunks";
  return coded_fault_of(c.frame, c.compression, c.chunks.data(), c.chunks.size(), c.bytes.data(), c.bytes.size(), g);
}

// The expansion: every chunk of a coded frame to its nominal size, as Frame::data holds them.  The records are checked here,
// the streams by the expanders themselves; false where coded_fault() would have refused.
inline bool unfax_all(const Coded& c, Frame& f, const char** why);
inline bool expand(const Coded& c, Frame& f) {
  if (ccitt::is_fax(c.compression)) return unfax_all(c, f, nullptr);  // a frame of parse_fax()
  Geometry g;
  if (!c.frame.data.empty() || detail::structure_fault(c.frame, c.compression, c.chunks.data(), c.chunks.size(), c.bytes.size(), g)) { f = Frame(); return false; }
  f = c.frame;
  f.data.assign(g.total, 0);  // (rows of a strip the image does not have stay zero)
  for (size_t k = 0; k < c.chunks.size(); ++k) {
    const uint8_t* s = c.bytes.data() + c.chunks[k].byte_off;
    const size_t len = c.chunks[k].byte_len, need = (size_t)c.chunks[k].rows * g.row_bytes;
    uint8_t* out = f.data.data() + k * g.chunk_bytes;
    bool ok;
    if (c.compression == 1) { ok = len >= need; if (ok) memcpy(out, s, need); }
    else if (c.compression == 32773) ok = detail::unpack_bits(s, len, out, need);
    else ok = detail::unlzw(s, len, out, need);
    if (!ok) { f = Frame(); return false; }
  }
  f.device_ok = c.chunks.size() <= kMaxDeviceChunks && g.total <= kMaxDeviceBytes;
  return true;
}

namespace detail {
// the coded chunks of a parsed head into one pool (an uncompressed chunk: the bytes its rows need, no more).  scan: with the
// extent scan of every stream (coded_fault); without, the records alone are checked - for a caller that expands at once, whose
// expanders refuse exactly what the scan refuses
inline void gather_bytes(const uint8_t* d, const Head& h, Coded& c) {
  c.compression = (int)h.comp;
  c.chunks.resize(h.chunks);
  size_t pool = 0;
  for (size_t k = 0; k < h.chunks; ++k) {
    const size_t rows = h.rows(c.frame, k), len = h.comp == 1 ? rows * h.g.row_bytes : h.len(k);
    c.chunks[k].byte_off = pool; c.chunks[k].byte_len = (uint32_t)len; c.chunks[k].rows = (uint32_t)rows;
    pool += len;
  }
  c.bytes.resize(pool);
  for (size_t k = 0; k < h.chunks; ++k) {
    const uint8_t* s = d + h.at(k);
    uint8_t* o = c.bytes.data() + c.chunks[k].byte_off;
    if (h.fill == 2) for (size_t i = 0; i < c.chunks[k].byte_len; ++i) o[i] = reverse_bits(s[i]);  // FillOrder 2: the coded bytes with their bits reversed
    else memcpy(o, s, c.chunks[k].byte_len);
  }
}
inline bool gather(const uint8_t* d, const Head& h, Coded& c, bool scan) {
  gather_bytes(d, h, c);
  Geometry g;
  if (scan ? coded_fault(c, g) : structure_fault(c.frame, c.compression, c.chunks.data(), c.chunks.size(), c.bytes.size(), g)) return false;
  c.frame.device_ok = h.chunks <= kMaxDeviceChunks && g.total <= kMaxDeviceBytes;
  return true;
}
}  // namespace detail

// The fax route (Compression 2, 3, 4 and 32771), reached by names of its own.  The rules of a fax frame over its parts
// (csrc/capi_tiff.hip runs the same text on its side of the ABI): fault(), what the coding asks of the frame, the records, and
// ccitt::walk over every chunk's stream with no output - the decoder's own verdict, found on the host, because the device
// expander cannot refuse a file.  nullptr when it is sound.
inline const char* fax_structure_fault(const Frame& f, int compression, uint32_t t4, const Chunk* chunks, size_t nchunks, size_t pool, Geometry& g) {
  if (const char* why = fault(f, g)) return why;
  if (!ccitt::is_fax(compression)) return "fax: compression must be 2, 3, 4 or 32771 (CCITT)";
  if (f.bits != 1 || f.samples != 1) return "fax: CCITT coding needs 1 bit per sample and 1 sample per pixel";
  if (f.photometric > 1) return "fax: CCITT coding needs photometric 0 or 1";
  if (f.predictor != 1) return "fax: CCITT coding takes no predictor";
  if (t4 & 2) return ccitt::kUncompressed;
  if ((t4 & ~7u) || (compression != 3 && t4)) return "fax: T4Options has bits beyond 0 .. 2, or belongs to another coding than Compression 3";
  return detail::records_fault(f, g, chunks, nchunks, pool);
}
inline const char* fax_fault_of(const Frame& f, int compression, uint32_t t4, const Chunk* chunks, size_t nchunks, const uint8_t* bytes, size_t pool, Geometry& g) {
  if (const char* why = fax_structure_fault(f, compression, t4, chunks, nchunks, pool, g)) return why;
  if (pool && !bytes) return "coded: the byte pool is missing";
  for (size_t c = 0; c < nchunks; ++c)
    if (const char* why = ccitt::walk(bytes + chunks[c].byte_off, chunks[c].byte_len, compression, t4, (uint32_t)f.tile_width, chunks[c].rows, nullptr, 0)) return why;
  return nullptr;
}
inline const char* fax_fault(const Coded& c, Geometry& g) {
  if (!c.frame.data.empty()) return "coded: a coded frame carries no expanded chunks";
  return fax_fault_of(c.frame, c.compression, c.t4_options, c.chunks.data(), c.chunks.size(), c.bytes.data(), c.bytes.size(), g);
}
// The host expansion of a fax frame: what parse() gives for the file.  false, with the reason at *why, where fax_fault() would
// have refused: the records are checked here, the streams by the decoder itself.
inline bool unfax_all(const Coded& c, Frame& f, const char** why = nullptr) {
  Geometry g;
  const char* w = !c.frame.data.empty() ? "coded: a coded frame carries no expanded chunks"
                                        : fax_structure_fault(c.frame, c.compression, c.t4_options, c.chunks.data(), c.chunks.size(), c.bytes.size(), g);
  if (!w) {
    f = c.frame;
    for (size_t k = 0; k < c.chunks.size() && !w; ++k) {
      f.data.resize((k + 1) * g.chunk_bytes, 0);  // (chunk by chunk, as parse() grows it; rows of a strip the image does not have stay zero)
      w = ccitt::walk(c.bytes.data() + c.chunks[k].byte_off, c.chunks[k].byte_len, c.compression, c.t4_options, (uint32_t)f.tile_width, c.chunks[k].rows,
                      f.data.data() + k * g.chunk_bytes, g.row_bytes);
    }
  }
  if (why) *why = w;
  if (w) { f = Frame(); return false; }
  f.device_ok = c.chunks.size() <= kMaxDeviceChunks && g.total <= kMaxDeviceBytes;
  return true;
}
namespace detail {
inline bool gather_fax(const uint8_t* d, const Head& h, Coded& c, bool scan, const char** why) {
  gather_bytes(d, h, c);
  c.t4_options = h.t4;
  Geometry g;
  const char* w = scan ? fax_fault(c, g) : fax_structure_fault(c.frame, c.compression, c.t4_options, c.chunks.data(), c.chunks.size(), c.bytes.size(), g);
  if (why) *why = w;
  if (w) return false;
  c.frame.device_ok = h.chunks <= kMaxDeviceChunks && g.total <= kMaxDeviceBytes;
  return true;
}
}  // namespace detail
// The container alone of a CCITT file: one Chunk per strip or tile, the coding and the T4 options, every stream scanned with the
// decoder's verdict - so that true means unfax_all(), on the host or on the device, has what it needs.  false: not such a
// file, or a refused one; *why then says which rule of the coding refused it (nullptr: the container did, or it is no fax file).
inline bool parse_fax(const uint8_t* d, size_t n, Coded& c, const char** why = nullptr) {
  c = Coded();
  if (why) *why = nullptr;
  detail::Head h;
  if (!detail::parse_head(d, n, c.frame, h)) { if (why) *why = h.why; c = Coded(); return false; }
  if (!ccitt::is_fax((int)h.comp) || !detail::gather_fax(d, h, c, true, why)) { c = Coded(); return false; }
  return true;
}

// The container alone, for the files whose expansion the device can take: Compression 1, 5 and 32773.  Every chunk's stream
// is scanned (coded_fault), so that kCoded means expand() - on the host or on the device - has what it needs.  Deflate answers
// kOtherRoute: parse() is the way.
inline Route parse_coded(const uint8_t* d, size_t n, Coded& c) {
  c = Coded();
  detail::Head h;
  if (!detail::parse_head(d, n, c.frame, h)) { c = Coded(); return kRefused; }
  if (ccitt::is_fax((int)h.comp)) {  // a sound CCITT file: parse_fax() is the way; an unsound one is refused here already
    const bool ok = detail::gather_fax(d, h, c, true, nullptr);
    c = Coded();
    return ok ? kFaxRoute : kRefused;
  }
  if (h.comp != 1 && h.comp != 5 && h.comp != 32773) { c = Coded(); return kOtherRoute; }
  if (!detail::gather(d, h, c, true)) { c = Coded(); return kRefused; }
  return kCoded;
}

// The Deflate route (Compression 8 / 32946), reached by names of its own: the container alone - no stream is looked at, the
// device's inflate kernel (csrc/kernels_inflate.hip) gives the verdict per chunk, and inflate_all() is the host's.
inline const char* deflate_fault_of(const Frame& f, int compression, const Chunk* chunks, size_t nchunks, const uint8_t* bytes, size_t pool, Geometry& g) {
  if (const char* why = detail::structure_fault(f, compression, chunks, nchunks, pool, g, true)) return why;
  if (pool && !bytes) return "coded: the byte pool is missing";
  return nullptr;
}
inline bool parse_deflate(const uint8_t* d, size_t n, Coded& c) {
  c = Coded();
  detail::Head h;
  if (!detail::parse_head(d, n, c.frame, h) || (h.comp != 8 && h.comp != 32946)) { c = Coded(); return false; }
  c.compression = (int)h.comp;
  detail::gather_bytes(d, h, c);
  Geometry g;
  if (deflate_fault_of(c.frame, c.compression, c.chunks.data(), c.chunks.size(), c.bytes.data(), c.bytes.size(), g)) { c = Coded(); return false; }
  c.frame.device_ok = h.chunks <= kMaxDeviceChunks && g.total <= kMaxDeviceBytes;
  return true;
}
// parse_coded() and parse_deflate() behind one reading of the container: kCoded with `deflate` false is parse_coded()'s answer,
// kCoded with `deflate` true parse_deflate()'s; kFaxRoute is parse_fax()'s true, with the fax frame in c - with scan_fax false its
// streams have not been walked, for a caller that goes on to unfax_all(), which gives the same verdict; kOtherRoute does not
// occur.  why: as parse_fax's.
inline Route parse_any(const uint8_t* d, size_t n, Coded& c, bool& deflate, bool scan_fax = true, const char** why = nullptr) {
  c = Coded();
  if (why) *why = nullptr;
  detail::Head h;
  if (!detail::parse_head(d, n, c.frame, h)) { if (why) *why = h.why; c = Coded(); return kRefused; }
  if (ccitt::is_fax((int)h.comp)) {
    deflate = false;
    if (!detail::gather_fax(d, h, c, scan_fax, why)) { c = Coded(); return kRefused; }
    return kFaxRoute;
  }
  deflate = h.comp == 8 || h.comp == 32946;
  if (!deflate) {
    if (!detail::gather(d, h, c, true)) { c = Coded(); return kRefused; }
    return kCoded;
  }
  detail::gather_bytes(d, h, c);
  Geometry g;
  if (deflate_fault_of(c.frame, c.compression, c.chunks.data(), c.chunks.size(), c.bytes.data(), c.bytes.size(), g)) { c = Coded(); return kRefused; }
  c.frame.device_ok = h.chunks <= kMaxDeviceChunks && g.total <= kMaxDeviceBytes;
  return kCoded;
}
// The host expansion of such a frame: what parse() gives for the file.  false where a chunk's stream does not hold its bytes.
inline bool inflate_all(const Coded& c, Frame& f) {
  Geometry g;
  if (!c.frame.data.empty() || deflate_fault_of(c.frame, c.compression, c.chunks.data(), c.chunks.size(), c.bytes.data(), c.bytes.size(), g)) { f = Frame(); return false; }
  f = c.frame;
  for (size_t k = 0; k < c.chunks.size(); ++k) {
    f.data.resize((k + 1) * g.chunk_bytes, 0);  // (chunk by chunk, as parse() grows it)
    if (!detail::inflate(c.bytes.data() + c.chunks[k].byte_off, c.chunks[k].byte_len, f.data.data() + k * g.chunk_bytes, (size_t)c.chunks[k].rows * g.row_bytes)) { f = Frame(); return false; }
  }
  f.device_ok = c.chunks.size() <= kMaxDeviceChunks && g.total <= kMaxDeviceBytes;
  return true;
}

// The container and the expansion: everything but the pixels.  false = not a TIFF file, or one that is refused.
inline bool parse(const uint8_t* d, size_t n, Frame& f, const char** why = nullptr) {
  using namespace detail;
  Head h;
  if (why) *why = nullptr;
  if (!parse_head(d, n, f, h)) { if (why) *why = h.why; return false; }
  if (ccitt::is_fax((int)h.comp)) {
    Coded c;  // parse_fax + unfax_all, less the scan: the decoder refuses what its scan refuses
    c.frame = f;
    if (!gather_fax(d, h, c, false, why) || !unfax_all(c, f, why)) { f = Frame(); return false; }
    return true;
  }
  if (h.comp == 1 || h.comp == 5 || h.comp == 32773) {
    Coded c;  // parse_coded + expand, less the scan: unlzw / unpack_bits refuse what lzw_extent / packbits_extent refuse
    c.frame = f;
    if (!gather(d, h, c, false) || !expand(c, f)) { f = Frame(); return false; }
    return true;
  }
  const Geometry& g = h.g;
  std::vector<uint8_t> turned;  // FillOrder 2: the coded bytes of a chunk with their bits reversed
  for (size_t c = 0; c < h.chunks; ++c) {
    const size_t len = h.len(c), need = h.rows(f, c) * g.row_bytes;
    const uint8_t* s = d + h.at(c);
    if (h.fill == 2) {
      turned.resize(len);
      for (size_t i = 0; i < len; ++i) turned[i] = reverse_bits(s[i]);
      s = turned.data();
    }
    // the buffer grows chunk by chunk - a header's claim alone allocates nothing - to g.total at most
    f.data.resize((c + 1) * g.chunk_bytes, 0);
    if (!inflate(s, len, f.data.data() + c * g.chunk_bytes, need)) { f = Frame(); return false; }
  }
  f.device_ok = h.chunks <= kMaxDeviceChunks && g.total <= kMaxDeviceBytes;
  return true;
}

namespace detail {
// one pixel from its (accumulated) samples v[0 .. used): o = B, G, R
inline void convert(const Frame& f, const uint32_t* v, uint8_t* o) {
  const int ph = f.photometric;
  if (ph == 3) { memcpy(o, f.palette + 4 * (v[0] & 255), 3); return; }
  if (ph == 5) {
    const uint32_t k = 255 - v[3];
    o[2] = (uint8_t)(k * (255 - v[0]) / 255); o[1] = (uint8_t)(k * (255 - v[1]) / 255); o[0] = (uint8_t)(k * (255 - v[2]) / 255);
    return;
  }
  if (ph <= 1 && f.planar == 1) {
    uint32_t c = f.bits == 16 ? v[0] >> 8 : f.bits == 8 ? v[0] : v[0] * 255 / ((1u << f.bits) - 1);
    if (ph == 0) c = 255 - c;
    o[0] = o[1] = o[2] = (uint8_t)c;
    return;
  }
  // RGB, and grey in planes
  const int nc = ph == 2 ? 3 : 1;
  uint32_t c[4];
  for (int i = 0; i <= nc; ++i) c[i] = f.bits == 16 ? (v[i] + 128) / 257 : v[i];  // (c[nc]: alpha, read only when it premultiplies)
  if (f.premultiply)
    for (int i = 0; i < nc; ++i) c[i] = (c[i] * c[nc] + 127) / 255;
  if (nc == 3) { o[0] = (uint8_t)c[2]; o[1] = (uint8_t)c[1]; o[2] = (uint8_t)c[0]; }
  else o[0] = o[1] = o[2] = (uint8_t)c[0];
}
}  // namespace detail

// The pixel half on the host: undo the predictor, convert, place.  bgr: height x width x 3.  false on a frame that parse()
// would not have produced.
inline bool pixels(const Frame& f, std::vector<uint8_t>& bgr) {
  Geometry g;
  if (!sound(f, g)) return false;
  bgr.resize((size_t)f.width * f.height * 3);
  const int used = g.used, bytes = f.bits == 16 ? 2 : 1;
  const uint32_t mask = f.bits == 16 ? 0xFFFFu : 0xFFu;
  const size_t plane = f.planar == 2 ? g.chunk_bytes * g.across * g.down : 0;
  for (int cy = 0; cy < g.down; ++cy)
    for (int cx = 0; cx < g.across; ++cx) {
      const int cols = f.width - cx * f.tile_width < f.tile_width ? f.width - cx * f.tile_width : f.tile_width;
      const int rows = f.height - cy * f.tile_height < f.tile_height ? f.height - cy * f.tile_height : f.tile_height;
      const uint8_t* chunk = f.data.data() + ((size_t)cy * g.across + cx) * g.chunk_bytes;
      for (int y = 0; y < rows; ++y) {
        const uint8_t* row = chunk + (size_t)y * g.row_bytes;
        uint8_t* o = bgr.data() + (((size_t)cy * f.tile_height + y) * f.width + (size_t)cx * f.tile_width) * 3;
        uint32_t sum[4] = {0, 0, 0, 0}, v[4] = {0, 0, 0, 0};
        for (int x = 0; x < cols; ++x, o += 3) {
          if (f.bits < 8) {
            const int per = 8 / f.bits;
            v[0] = (row[x / per] >> ((per - 1 - x % per) * f.bits)) & ((1u << f.bits) - 1);
          } else {
            for (int k = 0; k < used; ++k) {
              const uint8_t* s = f.planar == 2 ? row + k * plane + (size_t)x * bytes : row + ((size_t)x * f.samples + k) * bytes;
              uint32_t t = bytes == 1 ? s[0] : f.big_endian ? ((uint32_t)s[0] << 8) | s[1] : (uint32_t)s[0] | ((uint32_t)s[1] << 8);
              if (f.predictor == 2) t = sum[k] = (sum[k] + t) & mask;
              v[k] = t;
            }
          }
          detail::convert(f, v, o);
        }
      }
    }
  return true;
}

}  // namespace tiff
}  // namespace PaddleOCR
