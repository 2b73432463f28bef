// JPEG 2000 (Part 1: a JP2 file or a bare codestream) decoder in two halves, shaped like vp8_decode.h: whatever is serial on
// the caller's host thread - parse() - and the sample arithmetic either on the device (csrc/kernels_j2k.hip, through
// ocr_j2k_frame) or here - pixels().
//
// What comes out is what cv::imdecode(data, IMREAD_COLOR) returns for such a file: OpenJPEG's samples (OpenCV >= 4.3 reads
// JPEG 2000 through it), one colour channel replicated to B = G = R, three written B, G, R, alpha dropped, a precision above 8
// reduced by >> (prec - 8).  tests/test_j2k_decode.py compares with the OpenJPEG that Pillow bundles.
//
// Container: the 12-byte signature box, then boxes with 32-bit lengths, 0 (to the end of the file) and 1 (XLBox, 64 bits);
// "ftyp" is skipped like every unknown box; "jp2h" holds "ihdr", "bpcc" (read past), "colr" (method 1: sRGB 16 and greyscale 17,
// others refused; method 2, an ICC profile, is ignored as OpenJPEG's decoder ignores it) and "cdef" (which component is which
// colour, and which is alpha); "pclr" / "cmap" refuse the file; the first "jp2c" is the image.  A bare codestream starts
// ff 4f ff 51 and its colour space is guessed from the component count (1 or 2: grey, 3 or 4: RGB).
//
// Codestream: SIZ, COD, COC, QCD, QCC in the main header and in tile-part headers, SOT / SOD with any number of tile-parts per
// tile (their bodies are decoded as one sequence of packets), EOC; COM, TLM, PLM, PLT, CRG are skipped.  Tier-2: the five
// progression orders, layers, precincts, tag trees, number of passes, Lblock, lengths, SOP / EPH when COD announces them.
// Tier-1: the MQ decoder and the three passes of code-block style 0.  Refused, each with a reason (Frame::error): any code-block
// style bit, HT code blocks, POC, PPM, PPT, RGN, palettes, other colour spaces, signed components, more than 4 components,
// components of differing size or precision, subsampling, precision above 16, geometry beyond kMaxPixels.
//
// The frame descriptor (Frame; ocr_j2k_frame of include/ocr_hip.h states the same): per tile and carried component a
// TileComp - its rectangle on the reference grid, its decomposition levels, where its coefficients and step sizes lie - and
// ONE int32 array of coefficients, (x1 - x0) * (y1 - y0) per tile-component in the band arrangement: resolution r occupies the
// top-left corner of the rectangle, LL / LH on the left, HL / HH on the right, as wide and high as band_rect() says.  A
// band's rectangle and the parity of its origin follow from the tile-component rectangle by the standard's formula
// (band_rect, res_rect: stated once, for host and device), so they are derived, not carried twice.  A coefficient is tier-1's
// integer WITH its half bit: sign * (2 * magnitude + 1) << (undecoded planes) in units of half a quantiser step.
//
// Pixel half, pixels(), and kernels_j2k.hip after it (OpenJPEG 2.5's arithmetic, found out against the library):
//   - dequantise: 5/3: v / 2, truncating towards zero; 9/7: (float)v * (0.5f * step), step = (float)((1 + mant / 2048) *
//     2^(prec - expn)) (no band gain on the 9/7 path)
//   - inverse DWT resolution by resolution, rows first, columns second.  Low-pass samples are those at EVEN coordinates of the
//     tile-component's resolution grid, so the parity of the origin (image offset, tile offset, tile boundaries) decides which
//     comes first; a neighbour beyond the edge is the sample on the other side (symmetric extension by one).  5/3 in wrapping
//     int32: even -= (l + r + 2) >> 2, then odd += (l + r) >> 1; a row or column of ONE sample is copied at an even coordinate
//     and HALVED (truncating) at an odd one.  9/7 in float32 without contraction: even *= K, odd *= 2 / K (the doubled high-pass gain stands in for the band gain that step leaves out), then x += (l + r) * c
//     on even, odd, even, odd samples with c = -delta, -gamma, -beta, -alpha; a single sample is left untouched by the 9/7
//   - inverse component transform when COD says so: RCT (5/3) in int32, ICT (9/7) in float32
//   - 9/7: round to nearest even; add 1 << (prec - 1), clamp to [0, 2^prec - 1], >> (prec - 8) above 8 bits
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

// the pixel half's arithmetic is stated once: csrc/kernels_j2k.hip compiles these functions for the device too
#ifdef __HIPCC__
#define J2K_FN __host__ __device__ inline
#else
#define J2K_FN inline
#endif

namespace PaddleOCR {
namespace j2k {

constexpr long kMaxPixels = 64L << 20;  // the cap of the service's other decoders (kMaxDecodedPixels)
constexpr int kMaxLevels = 32;
constexpr int kMaxComps = 4;
constexpr float kK = 1.230174105f, kTwoInvK = 1.625732422f;
constexpr float kAlpha = -1.586134342f, kBeta = -0.052980118f, kGamma = 0.882911075f, kDelta = 0.443506852f;

struct Rect { int x0, y0, x1, y1; };

struct TileComp {  // ocr_j2k_tilecomp of include/ocr_hip.h, field for field
  int x0, y0, x1, y1;   // on the reference grid (no subsampling: the component's own)
  int levels;           // 0 .. 32
  int comp;             // the file's component index (informative)
  uint32_t step_off;    // into steps: 1 + 3 * levels values - LL, then HL, LH, HH of resolution 1, 2, ...
  uint32_t reserved;
  uint64_t coeff_off;   // into coeffs
};
static_assert(sizeof(TileComp) == 40, "TileComp is part of the C ABI");

struct Frame {
  int width = 0, height = 0;  // of the image: x1 - x0, y1 - y0
  int x0 = 0, y0 = 0;         // the image's origin on the reference grid
  int ncomp = 0;              // carried components per tile: 1 or 3
  int prec = 0;               // 1 .. 16
  int transform = 0;          // 0: 5/3 (reversible), 1: 9/7
  int mct = 0;                // the inverse component transform runs over the three carried components
  int chan[3] = {0, 0, 0};    // which carried component is R, G, B
  std::vector<TileComp> tcs;  // tile-major: ncomp records a tile
  std::vector<float> steps;
  std::vector<int32_t> coeffs;
  bool device_ok = false;     // within what the device stage takes (device_fault)
  // informative: what the file used
  int progression = 0, layers = 0, tiles_x = 0, tiles_y = 0, file_comps = 0, jp2 = 0, qstyle = 0, cbw = 0, cbh = 0, precincts = 0, tileparts = 0, sop = 0, eph = 0;
  const char* error = nullptr;  // why parse() refused (nullptr: a bare decode failure)
};

// The frame BEFORE tier-1 (parse_coded): the frame without its coefficients, every coded block with where its samples go, and
// the blocks' bytes.  What is left to do has no serial part: a block depends on no other (tier1(), or the device).
struct CodedBlock {  // ocr_j2k_cblk of include/ocr_hip.h, field for field
  uint32_t tc;        // index into Frame::tcs
  uint32_t at;        // sample offset of the block's top-left corner within its tile-component's plane (row stride x1 - x0)
  uint64_t byte_off;  // into Coded::bytes
  uint32_t byte_len;  // the block's chunks one after another, in layer order
  uint16_t w, h;      // 1 .. 1024 each, w * h <= 4096
  uint8_t orient;     // 0 LL, 1 HL, 2 LH, 3 HH
  uint8_t numbps;     // magnitude bit planes, 1 .. 30
  uint8_t passes;     // coding passes, 1 .. 3 * numbps - 2
  uint8_t reserved;
  uint32_t reserved2;
};
static_assert(sizeof(CodedBlock) == 32, "CodedBlock is part of the C ABI");
struct Coded {
  Frame frame;          // coeffs stays empty
  size_t ncoeffs = 0;   // what tier-1 fills: the sum of the tile-components' planes
  std::vector<CodedBlock> cblks;
  std::vector<uint8_t> bytes;
};

// ------------------------------------------------------------------------------------------------------------- geometry
J2K_FN int ceil_shift(int64_t a, int b) { return (int)((a + (((int64_t)1 << b) - 1)) >> b); }
// resolution with `lev` decompositions still to undo below the full size (lev = levels - r)
J2K_FN Rect res_rect(const Rect& tc, int lev) { return Rect{ceil_shift(tc.x0, lev), ceil_shift(tc.y0, lev), ceil_shift(tc.x1, lev), ceil_shift(tc.y1, lev)}; }
// band of decomposition level nb >= 1 (nb = levels - r + 1); orient 1 HL (x high-pass), 2 LH, 3 HH
J2K_FN Rect band_rect(const Rect& tc, int nb, int orient) {
  const int64_t ox = (orient & 1) ? ((int64_t)1 << (nb - 1)) : 0, oy = (orient & 2) ? ((int64_t)1 << (nb - 1)) : 0;
  return Rect{ceil_shift(tc.x0 - ox, nb), ceil_shift(tc.y0 - oy, nb), ceil_shift(tc.x1 - ox, nb), ceil_shift(tc.y1 - oy, nb)};
}

// ------------------------------------------------------------------------------------------------------------ arithmetic
J2K_FN int32_t wadd(int32_t a, int32_t b) { return (int32_t)((uint32_t)a + (uint32_t)b); }
J2K_FN int32_t wsub(int32_t a, int32_t b) { return (int32_t)((uint32_t)a - (uint32_t)b); }
J2K_FN int32_t half_trunc(int32_t v) { return v / 2; }
J2K_FN float bits_float(int32_t v) { union { int32_t i; float f; } u; u.i = v; return u.f; }
J2K_FN int32_t float_bits(float v) { union { int32_t i; float f; } u; u.f = v; return u.i; }
// a working sample is an int32: the integer itself (5/3) or the bits of a float (9/7)
J2K_FN int32_t dequant(int32_t v, int transform, float step) { return transform ? float_bits((float)v * (0.5f * step)) : half_trunc(v); }
J2K_FN int32_t lift53_even(int32_t x, int32_t l, int32_t r) { return wsub(x, wadd(wadd(l, r), 2) >> 2); }
J2K_FN int32_t lift53_odd(int32_t x, int32_t l, int32_t r) { return wadd(x, wadd(l, r) >> 1); }
J2K_FN float lift97(float x, float l, float r, float c) { return x + (l + r) * c; }
J2K_FN int32_t round_sample(float v) {
  if (!(v > -1.0e9f)) return -1000000000;  // NaN too
  if (v > 1.0e9f) return 1000000000;
#ifdef __HIP_DEVICE_COMPILE__
  return __float2int_rn(v);
#else
  return (int32_t)std::nearbyintf(v);  // to nearest even (the default rounding mode)
#endif
}
// three working samples of a pixel (s[1], s[2] unused without mct when ncomp == 1) -> the three colour samples 0 .. 255
J2K_FN void finish(const int32_t s[3], int ncomp, int transform, int mct, int prec, const int chan[3], uint8_t bgr[3]) {
  int32_t v[3] = {0, 0, 0};
  if (transform) {
    float f[3] = {bits_float(s[0]), ncomp > 1 ? bits_float(s[1]) : 0.f, ncomp > 1 ? bits_float(s[2]) : 0.f};
    if (mct && ncomp == 3) {
      const float y = f[0], u = f[1], w = f[2];
      f[0] = y + (w * 1.402f);
      f[1] = y - (u * 0.34413f) - (w * 0.71414f);
      f[2] = y + (u * 1.772f);
    }
    for (int k = 0; k < ncomp; ++k) v[k] = round_sample(f[k]);
  } else {
    for (int k = 0; k < ncomp; ++k) v[k] = s[k];
    if (mct && ncomp == 3) {
      const int32_t y = v[0], u = v[1], w = v[2];
      const int32_t g = wsub(y, wadd(u, w) >> 2);
      v[0] = wadd(w, g); v[1] = g; v[2] = wadd(u, g);
    }
  }
  const int32_t top = (1 << prec) - 1, shift = 1 << (prec - 1), down = prec > 8 ? prec - 8 : 0;
  for (int k = 0; k < 3; ++k) {
    int64_t x = (int64_t)v[chan[k]] + shift;
    x = x < 0 ? 0 : x > top ? top : x;
    bgr[2 - k] = (uint8_t)(x >> down);
  }
}

// why pixels() (and the device stage, which states the same rules over ocr_j2k_frame) refuses a frame; nullptr when sound
inline const char* fault_of(int width, int height, int x0, int y0, int ncomp, int prec, int transform, int mct, const int chan[3], const TileComp* tcs, size_t ntcs,
                            size_t nsteps, size_t ncoeffs) {
  if (width < 1 || height < 1 || (long)width * height > kMaxPixels) return "j2k frame: width and height must be positive and their product at most 64 Mi";
  if (x0 < 0 || y0 < 0 || (int64_t)x0 + width > 0x7fffffff || (int64_t)y0 + height > 0x7fffffff) return "j2k frame: the image origin must be non-negative";
  if (ncomp != 1 && ncomp != 3) return "j2k frame: 1 or 3 carried components";
  if (prec < 1 || prec > 16) return "j2k frame: precision must be 1 .. 16";
  if (transform < 0 || transform > 1 || mct < 0 || mct > 1) return "j2k frame: transform and mct must be 0 or 1";
  if (mct && ncomp != 3) return "j2k frame: the component transform takes three components";
  for (int k = 0; k < 3; ++k)
    if (chan[k] < 0 || chan[k] >= ncomp) return "j2k frame: channel map beyond the carried components";
  if (!tcs || ntcs == 0 || ntcs % (size_t)ncomp) return "j2k frame: tile-component records must come ncomp a tile";
  // the tiles must cover the image exactly once: each inside it, their areas adding up to it, in raster order without overlap
  int64_t area = 0;
  int prev_x1 = x0, prev_y0 = y0, prev_y1 = y0;
  for (size_t t = 0; t < ntcs; t += (size_t)ncomp) {
    const TileComp& a = tcs[t];
    if (a.x0 < x0 || a.y0 < y0 || a.x1 > x0 + width || a.y1 > y0 + height || a.x0 >= a.x1 || a.y0 >= a.y1) return "j2k frame: a tile lies outside the image";
    if (a.x0 == x0) {  // a new row of tiles starts below the last one
      if (a.y0 != prev_y1 || (t && prev_x1 != x0 + width)) return "j2k frame: tiles must cover the image in raster order";
      prev_y0 = a.y0; prev_y1 = a.y1;
    } else if (a.x0 != prev_x1 || a.y0 != prev_y0 || a.y1 != prev_y1) {
      return "j2k frame: tiles must cover the image in raster order";
    }
    prev_x1 = a.x1;
    area += (int64_t)(a.x1 - a.x0) * (a.y1 - a.y0);
    for (int c = 0; c < ncomp; ++c) {
      const TileComp& b = tcs[t + (size_t)c];
      if (b.x0 != a.x0 || b.y0 != a.y0 || b.x1 != a.x1 || b.y1 != a.y1) return "j2k frame: the components of a tile must share its rectangle";
      if (b.levels < 0 || b.levels > kMaxLevels) return "j2k frame: decomposition levels must be 0 .. 32";
      if ((size_t)b.step_off + 1 + 3 * (size_t)b.levels > nsteps) return "j2k frame: step sizes lie beyond the array";
      if (b.coeff_off > ncoeffs || (uint64_t)(b.x1 - b.x0) * (uint64_t)(b.y1 - b.y0) > ncoeffs - b.coeff_off) return "j2k frame: coefficients lie beyond the array";
    }
  }
  if (area != (int64_t)width * height || prev_x1 != x0 + width || prev_y1 != y0 + height) return "j2k frame: tiles must cover the image in raster order";
  return nullptr;
}
inline const char* fault(const Frame& f) {
  return fault_of(f.width, f.height, f.x0, f.y0, f.ncomp, f.prec, f.transform, f.mct, f.chan, f.tcs.data(), f.tcs.size(), f.steps.size(), f.coeffs.size());
}
// what the device stage leaves to the host (nullptr: it takes the frame): its working planes are indexed with 32 bits, a
// batch's step list has one entry per level, and the components of a tile are finished together
constexpr int kDeviceMaxLevels = 8;
inline const char* device_fault(int width, int height, int ncomp, const TileComp* tcs, size_t ntcs) {
  if ((int64_t)width * height * ncomp > ((int64_t)1 << 28)) return "j2k frame: more samples than the device stage indexes";
  for (size_t t = 0; t < ntcs; ++t) {
    if (tcs[t].levels > kDeviceMaxLevels) return "j2k frame: more decomposition levels than the device stage runs";
    if (tcs[t].levels != tcs[t - t % (size_t)ncomp].levels) return "j2k frame: the device stage wants one level count per tile";
  }
  return nullptr;
}

// why tier1() (and the device's tier-1, over ocr_j2k_coded) refuses a block list; nullptr when sound.  The tile-components
// are those of a frame that passed fault_of().  Two blocks may overlap: they race on values, never out of bounds.
inline const char* coded_fault(const TileComp* tcs, size_t ntcs, const CodedBlock* cblks, size_t ncblks, size_t nbytes) {
  if (ncblks && !cblks) return "j2k coded: the block list is missing";
  for (size_t i = 0; i < ncblks; ++i) {
    const CodedBlock& k = cblks[i];
    if (k.w < 1 || k.h < 1 || k.w > 1024 || k.h > 1024 || (int)k.w * k.h > 4096) return "j2k coded: a block must be 1 .. 1024 on a side and at most 4096 samples";
    if (k.orient > 3) return "j2k coded: a block's orientation must be 0 .. 3";
    if (k.numbps < 1 || k.numbps > 30) return "j2k coded: a block's bit planes must be 1 .. 30";
    if (k.passes < 1 || k.passes > 3 * k.numbps - 2) return "j2k coded: a block's passes must be 1 .. 3 * numbps - 2";
    if (k.tc >= ntcs) return "j2k coded: a block's tile-component lies beyond the list";
    const int64_t W = (int64_t)tcs[k.tc].x1 - tcs[k.tc].x0, H = (int64_t)tcs[k.tc].y1 - tcs[k.tc].y0;
    if (W < 1 || H < 1 || (int64_t)k.at % W + k.w > W || (int64_t)k.at / W + k.h > H) return "j2k coded: a block's rectangle leaves its tile-component";
    if (k.byte_len > 0x7fffffffu || k.byte_off > nbytes || k.byte_len > nbytes - k.byte_off) return "j2k coded: a block's bytes lie beyond the pool";
  }
  return nullptr;
}

// ----------------------------------------------------------------------------------------------------------- the pixel half
namespace detail {

// one line of n samples whose first lies at coordinate u0, in place: the interleaved samples x[0 .. n)
inline void lift_line(int32_t* x, int n, int u0, int transform) {
  if (n == 1) {
    if (!transform && (u0 & 1)) x[0] = half_trunc(x[0]);
    return;
  }
  const int e0 = u0 & 1, o0 = 1 - e0;  // index of the first even / odd coordinate
  auto L = [&](int i) { return i > 0 ? i - 1 : i + 1; };
  auto R = [&](int i) { return i + 1 < n ? i + 1 : i - 1; };
  if (!transform) {
    for (int i = e0; i < n; i += 2) x[i] = lift53_even(x[i], x[L(i)], x[R(i)]);
    for (int i = o0; i < n; i += 2) x[i] = lift53_odd(x[i], x[L(i)], x[R(i)]);
    return;
  }
  float* f = reinterpret_cast<float*>(x);
  for (int i = e0; i < n; i += 2) f[i] = f[i] * kK;
  for (int i = o0; i < n; i += 2) f[i] = f[i] * kTwoInvK;
  const float c[4] = {-kDelta, -kGamma, -kBeta, -kAlpha};
  for (int s = 0; s < 4; ++s)
    for (int i = (s & 1) ? o0 : e0; i < n; i += 2) f[i] = lift97(f[i], f[L(i)], f[R(i)], c[s]);
}

// the inverse transform of one tile-component, in place over `p` (w x h, band arrangement in, samples out)
inline void idwt(int32_t* p, const Rect& tc, int levels, int transform, const float* steps) {
  const int w = tc.x1 - tc.x0, h = tc.y1 - tc.y0;
  // dequantise band by band
  for (int r = 0; r <= levels; ++r) {
    const Rect cur = res_rect(tc, levels - r);
    const int cw = cur.x1 - cur.x0, ch = cur.y1 - cur.y0;
    if (r == 0) {
      for (int y = 0; y < ch; ++y)
        for (int x = 0; x < cw; ++x) p[(size_t)y * w + x] = dequant(p[(size_t)y * w + x], transform, steps[0]);
      continue;
    }
    const Rect low = res_rect(tc, levels - r + 1);
    const int lw = low.x1 - low.x0, lh = low.y1 - low.y0;
    for (int y = 0; y < ch; ++y)
      for (int x = (y < lh ? lw : 0); x < cw; ++x) {
        const int orient = (x >= lw ? 1 : 0) | (y >= lh ? 2 : 0);
        p[(size_t)y * w + x] = dequant(p[(size_t)y * w + x], transform, steps[1 + 3 * (r - 1) + orient - 1]);
      }
  }
  std::vector<int32_t> line((size_t)std::max(w, h));
  constexpr int kStrip = 16;  // columns taken together on the vertical pass
  std::vector<int32_t> cols((size_t)h * kStrip);
  for (int r = 1; r <= levels; ++r) {
    const Rect cur = res_rect(tc, levels - r), low = res_rect(tc, levels - r + 1);
    const int cw = cur.x1 - cur.x0, ch = cur.y1 - cur.y0, lw = low.x1 - low.x0, lh = low.y1 - low.y0;
    if (cw < 1 || ch < 1) continue;
    // rows: low-pass samples sit at even coordinates
    for (int y = 0; y < ch; ++y) {
      int32_t* row = p + (size_t)y * w;
      int nl = 0, nh = 0;
      for (int i = 0; i < cw; ++i) line[(size_t)i] = ((cur.x0 + i) & 1) ? row[lw + nh++] : row[nl++];
      lift_line(line.data(), cw, cur.x0, transform);
      memcpy(row, line.data(), (size_t)cw * 4);
    }
    // columns
    for (int x = 0; x < cw; x += kStrip) {
      const int n = std::min(kStrip, cw - x);
      int nl = 0, nh = 0;
      for (int i = 0; i < ch; ++i) {
        const int32_t* src = p + (size_t)(((cur.y0 + i) & 1) ? lh + nh++ : nl++) * w + x;
        for (int k = 0; k < n; ++k) cols[(size_t)k * h + i] = src[k];
      }
      for (int k = 0; k < n; ++k) lift_line(cols.data() + (size_t)k * h, ch, cur.y0, transform);
      for (int i = 0; i < ch; ++i)
        for (int k = 0; k < n; ++k) p[(size_t)i * w + x + k] = cols[(size_t)k * h + i];
    }
  }
}

}  // namespace detail

// The pixel half on the host: packed BGR, height x width.  false: the descriptor breaks a rule (fault()).
inline bool pixels(const Frame& f, std::vector<uint8_t>& bgr) {
  if (fault(f)) return false;
  bgr.assign((size_t)f.width * f.height * 3, 0);
  std::vector<int32_t> work[3];
  for (size_t t = 0; t < f.tcs.size(); t += (size_t)f.ncomp) {
    const TileComp& a = f.tcs[t];
    const int w = a.x1 - a.x0, h = a.y1 - a.y0;
    for (int c = 0; c < f.ncomp; ++c) {
      const TileComp& b = f.tcs[t + (size_t)c];
      work[c].assign(f.coeffs.begin() + (ptrdiff_t)b.coeff_off, f.coeffs.begin() + (ptrdiff_t)(b.coeff_off + (uint64_t)w * h));
      detail::idwt(work[c].data(), Rect{b.x0, b.y0, b.x1, b.y1}, b.levels, f.transform, f.steps.data() + b.step_off);
    }
    for (int y = 0; y < h; ++y) {
      uint8_t* out = bgr.data() + ((size_t)(a.y0 - f.y0 + y) * f.width + (size_t)(a.x0 - f.x0)) * 3;
      for (int x = 0; x < w; ++x) {
        const size_t i = (size_t)y * w + x;
        const int32_t s[3] = {work[0][i], f.ncomp > 1 ? work[1][i] : 0, f.ncomp > 1 ? work[2][i] : 0};
        finish(s, f.ncomp, f.transform, f.mct, f.prec, f.chan, out + (size_t)x * 3);
      }
    }
  }
  return true;
}

// ---------------------------------------------------------------------------------------------------------- the serial half
inline bool is_j2k(const uint8_t* d, size_t n) {
  static const uint8_t kSig[12] = {0, 0, 0, 12, 'j', 'P', ' ', ' ', 13, 10, 0x87, 10};
  if (n >= 12 && !memcmp(d, kSig, 12)) return true;
  return n >= 4 && d[0] == 0xff && d[1] == 0x4f && d[2] == 0xff && d[3] == 0x51;
}

namespace detail {

inline uint32_t be16(const uint8_t* p) { return (uint32_t)(p[0] << 8 | p[1]); }
inline uint32_t be32(const uint8_t* p) { return (uint32_t)p[0] << 24 | (uint32_t)p[1] << 16 | (uint32_t)p[2] << 8 | p[3]; }

struct Cod {  // per component
  int levels = 0, xcb = 6, ycb = 6, style = 0, transform = 0;
  int ppx[kMaxLevels + 1], ppy[kMaxLevels + 1];
  bool from_coc = false;
};
struct Qnt {
  int style = 0, guard = 0, n = 0;
  uint16_t expn[3 * kMaxLevels + 1], mant[3 * kMaxLevels + 1];
  bool from_qcc = false;
};
struct Params {  // of the main header, copied per tile and overridden by the tile's own markers
  int progression = 0, layers = 1, mct = 0, sop = 0, eph = 0;
  bool have_cod = false, have_qcd = false;
  Cod cod[kMaxComps];
  Qnt qnt[kMaxComps];
};

}  // namespace detail

// ------------------------------------------------------------------------------------------------------------------ tier-1
// Tier-1 of one code block is stated ONCE, as templates over the block's storage S, and compiled twice: for the host over
// vectors (detail::T1 below) and for the device over LDS (csrc/kernels_j2k_t1.hip).  S provides
//   int flag(x, y), void set_flag(x, y, v)   the sample's flags; x in -1 .. w, y in -1 .. h (a border of one sample, never set)
//   uint32_t mag(x, y), void set_mag(x, y, m)
//   int cx(i), void set_cx(i, v)             MQ context i of 19: state << 1 | mps
//   int at(uint32_t i)                       byte i of the block's segment; 0xff at or beyond its end (which feeds ones)
//   void clear(), void clear_visited()       all flags, magnitudes to zero; VISITED off everywhere
//   int width(), int height()
enum : int { kSig = 1, kNeg = 2, kVisited = 4, kRefined = 8 };
constexpr int kCxAgg = 17, kCxUni = 18, kCxMag = 14, kCxCount = 19;

// the MQ arithmetic decoder's probability table (software conventions)
struct MqState { uint16_t qe; uint8_t nmps, nlps, sw; };
J2K_FN MqState mq_row(int i) {
  static constexpr MqState kMq[47] = {
    {0x5601, 1, 1, 1},    {0x3401, 2, 6, 0},    {0x1801, 3, 9, 0},    {0x0ac1, 4, 12, 0},   {0x0521, 5, 29, 0},   {0x0221, 38, 33, 0},
    {0x5601, 7, 6, 1},    {0x5401, 8, 14, 0},   {0x4801, 9, 14, 0},   {0x3801, 10, 14, 0},  {0x3001, 11, 17, 0},  {0x2401, 12, 18, 0},
    {0x1c01, 13, 20, 0},  {0x1601, 29, 21, 0},  {0x5601, 15, 14, 1},  {0x5401, 16, 14, 0},  {0x5101, 17, 15, 0},  {0x4801, 18, 16, 0},
    {0x3801, 19, 17, 0},  {0x3401, 20, 18, 0},  {0x3001, 21, 19, 0},  {0x2801, 22, 19, 0},  {0x2401, 23, 20, 0},  {0x2201, 24, 21, 0},
    {0x1c01, 25, 22, 0},  {0x1801, 26, 23, 0},  {0x1601, 27, 24, 0},  {0x1401, 28, 25, 0},  {0x1201, 29, 26, 0},  {0x1101, 30, 27, 0},
    {0x0ac1, 31, 28, 0},  {0x09c1, 32, 29, 0},  {0x08a1, 33, 30, 0},  {0x0521, 34, 31, 0},  {0x0441, 35, 32, 0},  {0x02a1, 36, 33, 0},
    {0x0221, 37, 34, 0},  {0x0141, 38, 35, 0},  {0x0111, 39, 36, 0},  {0x0085, 40, 37, 0},  {0x0049, 41, 38, 0},  {0x0025, 42, 39, 0},
    {0x0015, 43, 40, 0},  {0x0009, 44, 41, 0},  {0x0005, 45, 42, 0},  {0x0001, 45, 43, 0},  {0x5601, 46, 46, 0}};
  return kMq[i];
}

// the decoder's registers; pos never passes the segment's length (beyond it every byte reads ff, which does not advance)
struct Mq { uint32_t pos, a, c; int ct; };
template <class S> J2K_FN void mq_bytein(S& s, Mq& q) {
  if (s.at(q.pos) == 0xff) {
    if (s.at(q.pos + 1) > 0x8f) { q.c += 0xff00; q.ct = 8; }  // a marker: not consumed
    else { ++q.pos; q.c += (uint32_t)s.at(q.pos) << 9; q.ct = 7; }
  } else { ++q.pos; q.c += (uint32_t)s.at(q.pos) << 8; q.ct = 8; }
}
template <class S> J2K_FN void mq_init(S& s, Mq& q) {
  for (int i = 0; i < kCxCount; ++i) s.set_cx(i, 0);
  s.set_cx(0, 4 << 1); s.set_cx(kCxAgg, 3 << 1); s.set_cx(kCxUni, 46 << 1);
  q.pos = 0; q.a = 0x8000; q.ct = 0;
  q.c = (uint32_t)s.at(0) << 16;
  mq_bytein(s, q);
  q.c <<= 7;
  q.ct -= 7;
}
// at most 15 shifts: a >= qe >= 1 on entry and the loop ends at a >= 0x8000
template <class S> J2K_FN void mq_renorm(S& s, Mq& q) {
  do {
    if (q.ct == 0) mq_bytein(s, q);
    q.a <<= 1; q.c <<= 1; --q.ct;
  } while (q.a < 0x8000);
}
template <class S> J2K_FN int mq_decode(S& s, Mq& q, int cx) {
  const int v = s.cx(cx), mps = v & 1;
  const MqState r = mq_row(v >> 1);
  const uint32_t qe = r.qe;
  bool lps;  // the less probable symbol came out
  q.a -= qe;
  if ((q.c >> 16) < qe) {
    lps = q.a >= qe;
    q.a = qe;
  } else {
    q.c -= qe << 16;
    if (q.a & 0x8000) return mps;
    lps = q.a < qe;
  }
  s.set_cx(cx, lps ? (r.nlps << 1 | (mps ^ r.sw)) : (r.nmps << 1 | mps));
  mq_renorm(s, q);
  return lps ? 1 - mps : mps;
}

// the zero-coding context of a sample from how many of its horizontal (0 .. 2), vertical (0 .. 2) and diagonal (0 .. 4)
// neighbours are significant
J2K_FN int zc_ctx(int hz, int v, int d, int orient) {
  if (orient == 3) {
    const int hv = hz + v;
    if (d >= 3) return 8;
    if (d == 2) return hv >= 1 ? 7 : 6;
    if (d == 1) return hv >= 2 ? 5 : hv == 1 ? 4 : 3;
    return hv >= 2 ? 2 : hv;
  }
  if (orient == 1) { const int t = hz; hz = v; v = t; }
  if (hz == 2) return 8;
  if (hz == 1) return v >= 1 ? 7 : d >= 1 ? 6 : 5;
  if (v == 2) return 4;
  if (v == 1) return 3;
  return d >= 2 ? 2 : d;
}
// the sign's context and whether the decoded bit is flipped, from the neighbours' contributions hc, vc in -1 .. 1
J2K_FN int sign_ctx(int hc, int vc) {
  static constexpr uint8_t ctx[3][3] = {{13, 12, 11}, {10, 9, 10}, {11, 12, 13}};  // [h + 1][v + 1]
  return ctx[hc + 1][vc + 1];
}
J2K_FN int sign_flip(int hc, int vc) {
  static constexpr uint8_t flip[3][3] = {{1, 1, 1}, {1, 0, 0}, {0, 0, 0}};
  return flip[hc + 1][vc + 1];
}
// the pass order: a block starts with the cleanup pass of its top plane, then significance, refinement, cleanup per plane
enum : int { kPassSig = 0, kPassRef = 1, kPassClean = 2 };
J2K_FN void pass_first(int numbps, int& bp1, int& type) { bp1 = numbps; type = kPassClean; }
J2K_FN void pass_next(int& bp1, int& type) { if (++type == 3) { type = kPassSig; --bp1; } }
J2K_FN int max_passes(int numbps) { return 3 * numbps - 2; }

namespace t1 {
template <class S> J2K_FN int sig(S& s, int x, int y) { return s.flag(x, y) & kSig; }
template <class S> J2K_FN int zc(S& s, int x, int y, int orient) {
  return zc_ctx(sig(s, x - 1, y) + sig(s, x + 1, y), sig(s, x, y - 1) + sig(s, x, y + 1),
                sig(s, x - 1, y - 1) + sig(s, x + 1, y - 1) + sig(s, x - 1, y + 1) + sig(s, x + 1, y + 1), orient);
}
template <class S> J2K_FN bool any(S& s, int x, int y) {
  return ((s.flag(x - 1, y) | s.flag(x + 1, y) | s.flag(x, y - 1) | s.flag(x, y + 1) | s.flag(x - 1, y - 1) | s.flag(x + 1, y - 1) | s.flag(x - 1, y + 1) |
           s.flag(x + 1, y + 1)) & kSig) != 0;
}
template <class S> J2K_FN int contrib(S& s, int x, int y) { const int f = s.flag(x, y); return (f & kSig) ? ((f & kNeg) ? -1 : 1) : 0; }
J2K_FN int clamp1(int v) { return v < -1 ? -1 : v > 1 ? 1 : v; }
template <class S> J2K_FN void sign(S& s, Mq& q, int x, int y) {
  const int hc = clamp1(contrib(s, x - 1, y) + contrib(s, x + 1, y)), vc = clamp1(contrib(s, x, y - 1) + contrib(s, x, y + 1));
  const int bit = mq_decode(s, q, sign_ctx(hc, vc)) ^ sign_flip(hc, vc);
  s.set_flag(x, y, s.flag(x, y) | (bit ? (kSig | kNeg) : kSig));
}
// The coding passes of one block into S: `numbps` magnitude planes, `passes` coding passes.  Every loop is bounded by the
// descriptor: at most max_passes(30) = 88 passes, width * height samples a pass and at most four decoded symbols a sample;
// no byte sequence changes how often a loop runs, only what it decodes.
template <class S> J2K_FN void decode(S& s, int numbps, int passes, int orient) {
  const int w = s.width(), h = s.height();
  s.clear();
  Mq q;
  mq_init(s, q);
  int bp1, type;
  pass_first(numbps, bp1, type);
  for (int p = 0; p < passes && bp1 >= 1; ++p) {
    const uint32_t one = 1u << bp1, half = one >> 1, oph = one | half;
    for (int y0 = 0; y0 < h; y0 += 4) {
      const int y1 = y0 + 4 < h ? y0 + 4 : h;
      for (int x = 0; x < w; ++x) {
        if (type == kPassSig) {
          for (int y = y0; y < y1; ++y) {
            if ((s.flag(x, y) & kSig) || !any(s, x, y)) continue;
            if (mq_decode(s, q, zc(s, x, y, orient))) { sign(s, q, x, y); s.set_mag(x, y, oph); }
            s.set_flag(x, y, s.flag(x, y) | kVisited);
          }
        } else if (type == kPassRef) {
          for (int y = y0; y < y1; ++y) {
            const int f = s.flag(x, y);
            if ((f & (kSig | kVisited)) != kSig) continue;
            const int cx = (f & kRefined) ? kCxMag + 2 : any(s, x, y) ? kCxMag + 1 : kCxMag;
            if (mq_decode(s, q, cx)) s.set_mag(x, y, s.mag(x, y) + half); else s.set_mag(x, y, s.mag(x, y) - half);
            s.set_flag(x, y, f | kRefined);
          }
        } else {
          int y = y0;
          if (y0 + 4 <= h && !((s.flag(x, y0) | s.flag(x, y0 + 1) | s.flag(x, y0 + 2) | s.flag(x, y0 + 3)) & (kSig | kVisited)) && !any(s, x, y0) &&
              !any(s, x, y0 + 1) && !any(s, x, y0 + 2) && !any(s, x, y0 + 3)) {
            if (!mq_decode(s, q, kCxAgg)) continue;
            int run = mq_decode(s, q, kCxUni) << 1;
            run |= mq_decode(s, q, kCxUni);
            y = y0 + run;
            sign(s, q, x, y);
            s.set_mag(x, y, oph);
            ++y;
          }
          for (; y < y1; ++y) {
            if (s.flag(x, y) & (kSig | kVisited)) continue;
            if (mq_decode(s, q, zc(s, x, y, orient))) { sign(s, q, x, y); s.set_mag(x, y, oph); }
          }
        }
      }
    }
    if (type == kPassClean) s.clear_visited();
    pass_next(bp1, type);
  }
}
// what a sample's state comes to: the signed integer with its half bit
J2K_FN int32_t coefficient(int flag, uint32_t mag) {
  const int32_t m = (int32_t)(mag & 0x7fffffffu);
  return (flag & kNeg) ? -m : m;
}
}  // namespace t1

namespace detail {

// tier-1's storage on the host: one code block of w x h samples over `len` bytes at `data`
struct T1 {
  std::vector<uint8_t> fl;
  std::vector<uint32_t> mg;
  uint8_t ctx[kCxCount];
  const uint8_t* data = nullptr;
  uint32_t len = 0;
  int w = 0, h = 0, fw = 0;
  int width() const { return w; }
  int height() const { return h; }
  int flag(int x, int y) const { return fl[(size_t)(y + 1) * fw + x + 1]; }
  void set_flag(int x, int y, int v) { fl[(size_t)(y + 1) * fw + x + 1] = (uint8_t)v; }
  uint32_t mag(int x, int y) const { return mg[(size_t)y * w + x]; }
  void set_mag(int x, int y, uint32_t m) { mg[(size_t)y * w + x] = m; }
  int cx(int i) const { return ctx[i]; }
  void set_cx(int i, int v) { ctx[i] = (uint8_t)v; }
  int at(uint32_t i) const { return i < len ? data[i] : 0xff; }
  void clear() { fl.assign((size_t)fw * (h + 2), 0); mg.assign((size_t)w * h, 0); }
  void clear_visited() { for (auto& f : fl) f &= (uint8_t)~kVisited; }
  // out: the signed integers with their half bit, row stride `stride`
  void run(const uint8_t* bytes, uint32_t n, int numbps, int passes, int orient, int cw, int chh, int32_t* out, size_t stride) {
    data = bytes; len = n; w = cw; h = chh; fw = w + 2;
    t1::decode(*this, numbps, passes, orient);
    for (int y = 0; y < h; ++y)
      for (int x = 0; x < w; ++x) out[(size_t)y * stride + x] = t1::coefficient(flag(x, y), mag(x, y));
  }
};

// packet-header bit reader with bit stuffing after ff
struct Bio {
  const uint8_t* d;
  size_t n, pos;
  uint32_t buf = 0;
  int ct = 0;
  bool bad = false;
  Bio(const uint8_t* data, size_t len, size_t at) : d(data), n(len), pos(at) {}
  int bit() {
    if (ct == 0) {
      buf = (buf << 8) & 0xffff;
      ct = buf == 0xff00 ? 7 : 8;
      if (pos >= n) { bad = true; return 0; }
      buf |= d[pos++];
    }
    --ct;
    return (int)(buf >> ct) & 1;
  }
  uint32_t bits(int k) { uint32_t v = 0; while (k-- > 0) v = v << 1 | (uint32_t)bit(); return v; }
  void align() {
    if ((buf & 0xff) == 0xff) {
      if (pos >= n) { bad = true; return; }
      ++pos;
    }
    ct = 0;
    buf = 0;
  }
};

struct TagTree {
  struct Node { int parent, value, low; };
  std::vector<Node> nodes;
  void init(int w, int h) {
    nodes.clear();
    int lw = w, lh = h, base = 0;
    std::vector<int> bases, ws, hs;
    while (true) {
      bases.push_back(base); ws.push_back(lw); hs.push_back(lh);
      base += lw * lh;
      if (lw * lh <= 1) break;
      lw = (lw + 1) / 2; lh = (lh + 1) / 2;
    }
    nodes.resize((size_t)base);
    for (size_t l = 0; l < bases.size(); ++l)
      for (int y = 0; y < hs[l]; ++y)
        for (int x = 0; x < ws[l]; ++x)
          nodes[(size_t)(bases[l] + y * ws[l] + x)] = Node{l + 1 < bases.size() ? bases[l + 1] + (y / 2) * ws[l + 1] + x / 2 : -1, 0x7fffffff, 0};
  }
  bool decode(Bio& b, int leaf, int threshold) {
    int stack[40], sp = 0, node = leaf;
    while (nodes[(size_t)node].parent >= 0 && sp < 40) { stack[sp++] = node; node = nodes[(size_t)node].parent; }
    int low = 0;
    for (;;) {
      Node& nd = nodes[(size_t)node];
      if (low > nd.low) nd.low = low; else low = nd.low;
      while (low < threshold && low < nd.value && !b.bad) {
        if (b.bit()) nd.value = low; else ++low;
      }
      nd.low = low;
      if (sp == 0) break;
      node = stack[--sp];
    }
    return nodes[(size_t)node].value < threshold;
  }
};

struct Cblk {
  int x0, y0, x1, y1;       // band coordinates
  int numbps = 0, lblock = 3, passes = 0;
  bool included = false;
  int32_t first = -1, last = -1;  // chunks
};
struct Chunk { size_t off; uint32_t len; int32_t next; };
struct PrecBand {
  int cw = 0, ch = 0;
  std::vector<Cblk> cblks;
  TagTree incl, msb;
};
struct Band { Rect r; int orient, numbps; int ox, oy; };  // ox, oy: where the band starts in the tile-component's buffer
struct Res {
  Rect r;
  int pdx, pdy, pw, ph, px0, py0, nbands;
  Band band[3];
  std::vector<PrecBand> prec;  // pw * ph * nbands, precinct-major
};
struct Packet { int64_t key[4]; int comp, res, prec, layer; };

inline int floor_log2(uint32_t v) { int l = 0; while (v > 1) { v >>= 1; ++l; } return l; }

}  // namespace detail

// One tile: structure, tier-2 over `data` (the tile-parts' bodies one after another), then the blocks tier-1 is to decode, with
// their bytes, for the carried components.  `carried[c]`: the slot of component c among the carried ones, or -1.
inline bool decode_tile(Coded& cd, const detail::Params& P, int ncomps, const Rect& tile, const std::vector<uint8_t>& data, const int* carried, size_t tc_base,
                        const char*& error) {
  using namespace detail;
  Frame& f = cd.frame;
  auto fail = [&](const char* why) { error = why; return false; };
  std::vector<std::vector<Res>> comps((size_t)ncomps);
  int64_t npackets = 0;
  for (int c = 0; c < ncomps; ++c) {
    const Cod& cod = P.cod[c];
    const Qnt& q = P.qnt[c];
    if (q.style != 1 && q.n < 3 * cod.levels + 1) return fail("j2k: fewer quantisation steps than bands");
    comps[(size_t)c].resize((size_t)cod.levels + 1);
    for (int r = 0; r <= cod.levels; ++r) {
      Res& R = comps[(size_t)c][(size_t)r];
      R.r = res_rect(tile, cod.levels - r);
      R.pdx = cod.ppx[r]; R.pdy = cod.ppy[r];
      if (r > 0 && (R.pdx < 1 || R.pdy < 1)) return fail("j2k: a precinct exponent of 0 above the lowest resolution");
      R.px0 = (R.r.x0 >> R.pdx) << R.pdx; R.py0 = (R.r.y0 >> R.pdy) << R.pdy;
      R.pw = R.r.x0 == R.r.x1 ? 0 : (int)((((int64_t)ceil_shift(R.r.x1, R.pdx) << R.pdx) - R.px0) >> R.pdx);
      R.ph = R.r.y0 == R.r.y1 ? 0 : (int)((((int64_t)ceil_shift(R.r.y1, R.pdy) << R.pdy) - R.py0) >> R.pdy);
      npackets += (int64_t)R.pw * R.ph * P.layers;
      if (npackets > (int64_t)data.size()) return fail("j2k: more packets than the tile has bytes");
      R.nbands = r == 0 ? 1 : 3;
      const Rect low = r ? res_rect(tile, cod.levels - r + 1) : R.r;
      for (int b = 0; b < R.nbands; ++b) {
        Band& B = R.band[b];
        B.orient = r == 0 ? 0 : b + 1;
        B.r = r == 0 ? R.r : band_rect(tile, cod.levels - r + 1, B.orient);
        B.ox = (B.orient & 1) ? low.x1 - low.x0 : 0;
        B.oy = (B.orient & 2) ? low.y1 - low.y0 : 0;
        const int bi = r == 0 ? 0 : 3 * (r - 1) + b + 1;
        const int expn = q.style == 1 ? std::max(0, (int)q.expn[0] - (bi ? (bi - 1) / 3 : 0)) : q.expn[bi];
        B.numbps = expn + q.guard - 1;
        if (B.numbps > 30) return fail("j2k: more than 30 magnitude bit planes");
        if (B.numbps < 0) B.numbps = 0;
      }
      R.prec.resize((size_t)R.pw * R.ph * R.nbands);
      const int cbx = std::min(cod.xcb, r ? R.pdx - 1 : R.pdx), cby = std::min(cod.ycb, r ? R.pdy - 1 : R.pdy);
      for (int pj = 0; pj < R.ph; ++pj)
        for (int pi = 0; pi < R.pw; ++pi)
          for (int b = 0; b < R.nbands; ++b) {
            PrecBand& pb = R.prec[((size_t)pj * R.pw + pi) * R.nbands + b];
            const Band& B = R.band[b];
            // the precinct on the band's grid
            int64_t gx0 = (int64_t)R.px0 + ((int64_t)pi << R.pdx), gy0 = (int64_t)R.py0 + ((int64_t)pj << R.pdy);
            int64_t gx1 = gx0 + ((int64_t)1 << R.pdx), gy1 = gy0 + ((int64_t)1 << R.pdy);
            if (r) { gx0 = (gx0 + 1) >> 1; gy0 = (gy0 + 1) >> 1; gx1 = (gx1 + 1) >> 1; gy1 = (gy1 + 1) >> 1; }
            // (the halved grid of a band: ceil for HL / HH alike, as the precinct's origin is a multiple of two)
            const int x0 = (int)std::max<int64_t>(gx0, B.r.x0), y0 = (int)std::max<int64_t>(gy0, B.r.y0);
            const int x1 = (int)std::min<int64_t>(gx1, B.r.x1), y1 = (int)std::min<int64_t>(gy1, B.r.y1);
            if (x0 >= x1 || y0 >= y1) continue;
            const int cx0 = (x0 >> cbx) << cbx, cy0 = (y0 >> cby) << cby;
            pb.cw = (int)((((int64_t)ceil_shift(x1, cbx) << cbx) - cx0) >> cbx);
            pb.ch = (int)((((int64_t)ceil_shift(y1, cby) << cby) - cy0) >> cby);
            pb.cblks.resize((size_t)pb.cw * pb.ch);
            for (int j = 0; j < pb.ch; ++j)
              for (int i = 0; i < pb.cw; ++i) {
                Cblk& k = pb.cblks[(size_t)j * pb.cw + i];
                k.x0 = std::max(cx0 + (i << cbx), x0); k.y0 = std::max(cy0 + (j << cby), y0);
                k.x1 = (int)std::min<int64_t>((int64_t)cx0 + ((int64_t)(i + 1) << cbx), x1); k.y1 = (int)std::min<int64_t>((int64_t)cy0 + ((int64_t)(j + 1) << cby), y1);
              }
            pb.incl.init(pb.cw, pb.ch);
            pb.msb.init(pb.cw, pb.ch);
          }
    }
  }
  // the packet sequence
  std::vector<Packet> seq;
  seq.reserve((size_t)npackets);
  for (int c = 0; c < ncomps; ++c)
    for (int r = 0; r <= P.cod[c].levels; ++r) {
      const Res& R = comps[(size_t)c][(size_t)r];
      const int lev = P.cod[c].levels - r;
      for (int pj = 0; pj < R.ph; ++pj)
        for (int pi = 0; pi < R.pw; ++pi) {
          const int64_t ax = std::max<int64_t>(tile.x0, ((int64_t)(R.px0 >> R.pdx) + pi) << (R.pdx + lev));
          const int64_t ay = std::max<int64_t>(tile.y0, ((int64_t)(R.py0 >> R.pdy) + pj) << (R.pdy + lev));
          const int p = pj * R.pw + pi;
          for (int l = 0; l < P.layers; ++l) {
            Packet k{{0, 0, 0, 0}, c, r, p, l};
            switch (P.progression) {
              case 0: k.key[0] = l; k.key[1] = r; k.key[2] = c; k.key[3] = p; break;                   // LRCP
              case 1: k.key[0] = r; k.key[1] = l; k.key[2] = c; k.key[3] = p; break;                   // RLCP
              case 2: k.key[0] = r; k.key[1] = ay; k.key[2] = ax; k.key[3] = ((int64_t)c << 20) + l; break;  // RPCL
              case 3: k.key[0] = ay; k.key[1] = ax; k.key[2] = c; k.key[3] = ((int64_t)r << 20) + l; break;  // PCRL
              default: k.key[0] = c; k.key[1] = ay; k.key[2] = ax; k.key[3] = ((int64_t)r << 20) + l; break; // CPRL
            }
            seq.push_back(k);
          }
        }
    }
  std::stable_sort(seq.begin(), seq.end(), [](const Packet& a, const Packet& b) {
    for (int i = 0; i < 4; ++i)
      if (a.key[i] != b.key[i]) return a.key[i] < b.key[i];
    return false;
  });
  // tier-2
  std::vector<Chunk> chunks;
  size_t pos = 0;
  const uint8_t* d = data.data();
  const size_t n = data.size();
  struct Got { Cblk* k; uint32_t len; };
  std::vector<Got> got;
  for (const Packet& pk : seq) {
    if (pos >= n) break;  // a tile cut short: what did not arrive stays zero
    Res& R = comps[(size_t)pk.comp][(size_t)pk.res];
    if (P.sop && pos + 6 <= n && d[pos] == 0xff && d[pos + 1] == 0x91) pos += 6;
    Bio bio(d, n, pos);
    got.clear();
    if (bio.bit()) {
      for (int b = 0; b < R.nbands; ++b) {
        PrecBand& pb = R.prec[(size_t)pk.prec * R.nbands + b];
        for (size_t ci = 0; ci < pb.cblks.size(); ++ci) {
          Cblk& k = pb.cblks[ci];
          bool inc;
          if (!k.included) inc = pb.incl.decode(bio, (int)ci, pk.layer + 1);
          else inc = bio.bit() != 0;
          if (bio.bad) return fail("j2k: a packet header runs beyond the tile's data");
          if (!inc) continue;
          if (!k.included) {
            int i = 1;
            while (!pb.msb.decode(bio, (int)ci, i)) {
              if (bio.bad || ++i > 64) return fail("j2k: a packet header runs beyond the tile's data");
            }
            k.numbps = R.band[b].numbps + 1 - i;
            if (k.numbps < 0) return fail("j2k: a code block with more zero bit planes than the band has planes");
            k.lblock = 3;
            k.included = true;
          }
          int np;
          if (!bio.bit()) np = 1;
          else if (!bio.bit()) np = 2;
          else if ((np = (int)bio.bits(2)) != 3) np += 3;
          else if ((np = (int)bio.bits(5)) != 31) np += 6;
          else np = 37 + (int)bio.bits(7);
          while (bio.bit()) {
            if (bio.bad || ++k.lblock > 32) return fail("j2k: a packet header runs beyond the tile's data");
          }
          const int nb = k.lblock + floor_log2((uint32_t)np);
          if (nb > 32) return fail("j2k: a code-block length of more than 32 bits");
          const uint32_t len = bio.bits(nb);
          if (bio.bad) return fail("j2k: a packet header runs beyond the tile's data");
          k.passes += np;
          got.push_back(Got{&k, len});
        }
      }
    }
    bio.align();
    if (bio.bad) return fail("j2k: a packet header runs beyond the tile's data");
    pos = bio.pos;
    if (P.eph) {
      if (pos + 2 <= n && d[pos] == 0xff && d[pos + 1] == 0x92) pos += 2;
      else return fail("j2k: a packet header does not end with the EPH marker COD announces");
    }
    for (const Got& g : got) {
      if (g.len > n - pos) return fail("j2k: a code block's bytes run beyond the tile's data");
      if (g.len) {
        chunks.push_back(Chunk{pos, g.len, -1});
        const int32_t id = (int32_t)chunks.size() - 1;
        if (g.k->last >= 0) chunks[(size_t)g.k->last].next = id; else g.k->first = id;
        g.k->last = id;
      }
      pos += g.len;
    }
  }
  // what tier-1 decodes, into the carried components' coefficients
  const int w = tile.x1 - tile.x0, h = tile.y1 - tile.y0;
  for (int c = 0; c < ncomps; ++c) {
    if (carried[c] < 0) continue;
    TileComp& tc = f.tcs[tc_base + (size_t)carried[c]];
    tc.x0 = tile.x0; tc.y0 = tile.y0; tc.x1 = tile.x1; tc.y1 = tile.y1;
    tc.levels = P.cod[c].levels;
    tc.comp = c;
    tc.reserved = 0;
    tc.step_off = (uint32_t)f.steps.size();
    tc.coeff_off = cd.ncoeffs;
    const Qnt& q = P.qnt[c];
    for (int bi = 0; bi < 3 * tc.levels + 1; ++bi) {
      const int expn = q.style == 1 ? std::max(0, (int)q.expn[0] - (bi ? (bi - 1) / 3 : 0)) : q.expn[bi];
      const int mant = q.style == 1 ? q.mant[0] : q.style == 2 ? q.mant[bi] : 0;
      f.steps.push_back((float)((1.0 + mant / 2048.0) * std::pow(2.0, f.prec - expn)));
    }
    cd.ncoeffs += (size_t)w * h;
    for (Res& R : comps[(size_t)c])
      for (size_t pi = 0; pi < R.prec.size(); ++pi) {
        const Band& B = R.band[pi % (size_t)R.nbands];
        for (const Cblk& k : R.prec[pi].cblks) {
          if (!k.included || k.passes == 0 || k.numbps == 0) continue;
          const size_t from = cd.bytes.size();
          for (int32_t id = k.first; id >= 0; id = chunks[(size_t)id].next) cd.bytes.insert(cd.bytes.end(), d + chunks[(size_t)id].off, d + chunks[(size_t)id].off + chunks[(size_t)id].len);
          if (cd.bytes.size() - from > 0x7fffffffu) return fail("j2k: a code block of more than 2 GiB");
          // (passes beyond max_passes are never run: t1::decode stops at the last plane)
          cd.cblks.push_back(CodedBlock{(uint32_t)(tc_base + (size_t)carried[c]), (uint32_t)((size_t)(B.oy + k.y0 - B.r.y0) * w + (size_t)(B.ox + k.x0 - B.r.x0)), from,
                                        (uint32_t)(cd.bytes.size() - from), (uint16_t)(k.x1 - k.x0), (uint16_t)(k.y1 - k.y0), (uint8_t)B.orient, (uint8_t)k.numbps,
                                        (uint8_t)std::min(k.passes, max_passes(k.numbps)), 0, 0});
        }
      }
  }
  return true;
}

// The serial half up to the seam between tier-2 and tier-1: container, headers, packets.  false: refused, Frame::error says
// why where a reason is known.
inline bool parse_coded(const uint8_t* d, size_t n, Coded& cd) {
  using namespace detail;
  cd = Coded();
  Frame& f = cd.frame;
  auto fail = [&](const char* why) { f.error = why; return false; };
  if (!is_j2k(d, n)) return fail("j2k: neither a JP2 signature nor a codestream");
  int colours = 0;              // 1 grey, 3 RGB; 0: guessed from the component count
  int cdef_n = 0;
  int cdef[16][3];
  if (d[0] == 0) {  // JP2: walk the boxes to the codestream
    f.jp2 = 1;
    size_t pos = 12, end = n;
    const uint8_t* cs = nullptr;
    size_t cs_len = 0;
    bool in_header = false;
    size_t header_end = 0;
    while (!cs) {
      if (in_header && pos >= header_end) { in_header = false; end = n; }
      if (pos + 8 > end) return fail("j2k: no codestream box");
      uint64_t len = be32(d + pos);
      const uint32_t type = be32(d + pos + 4);
      size_t hdr = 8;
      if (len == 1) {
        if (pos + 16 > end) return fail("j2k: a box header runs beyond the file");
        len = (uint64_t)be32(d + pos + 8) << 32 | be32(d + pos + 12);
        hdr = 16;
      } else if (len == 0) {
        len = end - pos;
      }
      if (len < hdr || len > end - pos) return fail("j2k: a box runs beyond the file");
      const uint8_t* body = d + pos + hdr;
      const size_t blen = (size_t)len - hdr;
      switch (type) {
        case 0x6a703268:  // jp2h: a superbox
          if (in_header) return fail("j2k: a header box inside the header box");
          in_header = true; header_end = pos + (size_t)len; end = header_end;
          pos += hdr;
          continue;
        case 0x6a703263:  // jp2c
          if (in_header) return fail("j2k: the codestream inside the header box");
          cs = body; cs_len = blen;
          break;
        case 0x70636c72: case 0x636d6170:  // pclr, cmap
          if (in_header) return fail("j2k: palette images are not decoded");
          break;
        case 0x636f6c72:  // colr
          if (in_header && !colours) {
            if (blen < 3) return fail("j2k: a colour box shorter than its fields");
            if (body[0] == 1) {
              if (blen < 7) return fail("j2k: a colour box shorter than its fields");
              const uint32_t e = be32(body + 3);
              if (e == 16) colours = 3;
              else if (e == 17) colours = 1;
              else return fail("j2k: only the sRGB and greyscale colour spaces are decoded");
            }
          }
          break;
        case 0x63646566:  // cdef
          if (in_header) {
            if (blen < 2 || blen < 2 + 6 * (size_t)be16(body) || be16(body) > 16) return fail("j2k: a channel definition box shorter than its entries");
            cdef_n = (int)be16(body);
            for (int i = 0; i < cdef_n; ++i)
              for (int k = 0; k < 3; ++k) cdef[i][k] = (int)be16(body + 2 + 6 * i + 2 * k);
          }
          break;
        default: break;  // ftyp, ihdr (SIZ says the same), bpcc, res, xml, uuid ...
      }
      pos += (size_t)len;
    }
    d = cs; n = cs_len;
    if (n < 4 || d[0] != 0xff || d[1] != 0x4f || d[2] != 0xff || d[3] != 0x51) return fail("j2k: the codestream box does not start with SOC and SIZ");
  }
  // ---- main header
  size_t pos = 2;
  auto seg_len = [&](size_t at) -> size_t { return at + 4 <= n ? be16(d + at + 2) : 0; };
  size_t L = seg_len(pos);
  if (L < 41 || pos + 2 + L > n) return fail("j2k: SIZ runs beyond the file");
  const uint8_t* s = d + pos + 4;
  const uint32_t rsiz = be16(s);
  if (rsiz & 0x4000) return fail("j2k: HT code blocks (Part 15) are not decoded");
  const uint32_t X = be32(s + 2), Y = be32(s + 6), XO = be32(s + 10), YO = be32(s + 14), XT = be32(s + 18), YT = be32(s + 22), XTO = be32(s + 26), YTO = be32(s + 30);
  const int ncomps = (int)be16(s + 34);
  if (ncomps < 1) return fail("j2k: no components");
  if (ncomps > kMaxComps) return fail("j2k: more than 4 components are not decoded");
  if (L != 38 + 3 * (size_t)ncomps) return fail("j2k: SIZ has another length than its component count asks");
  if (X > 0x7fffffffu || Y > 0x7fffffffu || XO >= X || YO >= Y || !XT || !YT || XT > 0x7fffffffu || YT > 0x7fffffffu || XTO > XO || YTO > YO ||
      (uint64_t)XTO + XT <= XO || (uint64_t)YTO + YT <= YO)
    return fail("j2k: image and tile geometry contradict each other");
  if ((uint64_t)(X - XO) * (uint64_t)(Y - YO) > (uint64_t)kMaxPixels) return fail("j2k: more than 64 Mi pixels");
  for (int c = 0; c < ncomps; ++c) {
    const uint8_t* cc = s + 36 + 3 * c;
    if (cc[0] & 0x80) return fail("j2k: signed components are not decoded");
    if (cc[1] != 1 || cc[2] != 1) return fail("j2k: subsampled components are not decoded");
    if (cc[0] != s[36]) return fail("j2k: components of differing precision are not decoded");
  }
  f.prec = (s[36] & 0x7f) + 1;
  if (f.prec > 16) return fail("j2k: a precision above 16 bits is not decoded");
  f.width = (int)(X - XO); f.height = (int)(Y - YO); f.x0 = (int)XO; f.y0 = (int)YO;
  f.file_comps = ncomps;
  const uint64_t tw = ((uint64_t)X - XTO + XT - 1) / XT, th = ((uint64_t)Y - YTO + YT - 1) / YT;
  if (tw * th > 65535 || tw * th * 14 > n) return fail("j2k: more tiles than the file has bytes for");
  f.tiles_x = (int)tw; f.tiles_y = (int)th;
  const size_t ntiles = (size_t)(tw * th);
  pos += 2 + L;

  Params main;
  // a marker segment of a main or tile-part header; false: refused
  auto header_marker = [&](uint32_t m, const uint8_t* b, size_t len, Params& P, bool in_tile) -> bool {
    auto spcod = [&](const uint8_t* p, size_t have, bool explicit_prec, Cod& c) -> bool {
      if (have < 5) return fail("j2k: a coding style segment shorter than its fields");
      c.levels = p[0];
      if (c.levels > kMaxLevels) return fail("j2k: more than 32 decomposition levels");
      c.xcb = (p[1] & 15) + 2; c.ycb = (p[2] & 15) + 2;
      if (c.xcb > 10 || c.ycb > 10 || c.xcb + c.ycb > 12) return fail("j2k: a code block larger than 4096 samples or 1024 on a side");
      c.style = p[3];
      if (c.style & 0x40) return fail("j2k: HT code blocks (Part 15) are not decoded");
      if (c.style) return fail("j2k: code-block styles (bypass, reset, termination, causal, segmentation symbols) are not decoded");
      if (p[4] > 1) return fail("j2k: an unknown wavelet transform");
      c.transform = p[4] == 0 ? 1 : 0;
      if (explicit_prec) {
        if (have < 5 + (size_t)c.levels + 1) return fail("j2k: a coding style segment shorter than its precincts");
        for (int r = 0; r <= c.levels; ++r) { c.ppx[r] = p[5 + r] & 15; c.ppy[r] = p[5 + r] >> 4; }
      } else {
        for (int r = 0; r <= kMaxLevels; ++r) c.ppx[r] = c.ppy[r] = 15;
      }
      return true;
    };
    auto sqcd = [&](const uint8_t* p, size_t have, Qnt& q) -> bool {
      if (have < 1) return fail("j2k: a quantisation segment shorter than its fields");
      q.style = p[0] & 31; q.guard = p[0] >> 5;
      if (q.style > 2) return fail("j2k: an unknown quantisation style");
      const size_t each = q.style == 0 ? 1 : 2;
      q.n = (int)std::min<size_t>((have - 1) / each, 3 * kMaxLevels + 1);
      if (q.n < 1) return fail("j2k: a quantisation segment without a step");
      for (int i = 0; i < q.n; ++i) {
        if (q.style == 0) { q.expn[i] = p[1 + i] >> 3; q.mant[i] = 0; }
        else { const uint32_t v = be16(p + 1 + 2 * i); q.expn[i] = (uint16_t)(v >> 11); q.mant[i] = v & 0x7ff; }
      }
      return true;
    };
    switch (m) {
      case 0xff52: {  // COD
        if (len < 10) return fail("j2k: a coding style segment shorter than its fields");
        P.sop = (b[0] >> 1) & 1; P.eph = (b[0] >> 2) & 1;
        P.progression = b[1];
        if (P.progression > 4) return fail("j2k: an unknown progression order");
        P.layers = (int)be16(b + 2);
        if (P.layers < 1) return fail("j2k: no quality layers");
        P.mct = b[4];
        if (P.mct > 1) return fail("j2k: an unknown component transform");
        Cod c;
        if (!spcod(b + 5, len - 5, b[0] & 1, c)) return false;
        for (int i = 0; i < ncomps; ++i)
          if (!P.cod[i].from_coc || (in_tile && !P.have_cod)) P.cod[i] = c;
        P.have_cod = true;
        return true;
      }
      case 0xff53: {  // COC
        if (len < 7 || b[0] >= ncomps) return fail("j2k: a component coding style segment for a component the image lacks");
        Cod c;
        if (!spcod(b + 2, len - 2, b[1] & 1, c)) return false;
        c.from_coc = true;
        P.cod[b[0]] = c;
        return true;
      }
      case 0xff5c: {  // QCD
        Qnt q;
        if (!sqcd(b, len, q)) return false;
        for (int i = 0; i < ncomps; ++i)
          if (!P.qnt[i].from_qcc) P.qnt[i] = q;
        P.have_qcd = true;
        return true;
      }
      case 0xff5d: {  // QCC
        if (len < 2 || b[0] >= ncomps) return fail("j2k: a component quantisation segment for a component the image lacks");
        Qnt q;
        if (!sqcd(b + 1, len - 1, q)) return false;
        q.from_qcc = true;
        P.qnt[b[0]] = q;
        return true;
      }
      case 0xff50: return fail("j2k: HT code blocks (Part 15) are not decoded");
      case 0xff5e: return fail("j2k: RGN (region of interest) is not decoded");
      case 0xff5f: return fail("j2k: POC (progression order changes) is not decoded");
      case 0xff60: return fail("j2k: PPM (packed packet headers) is not decoded");
      case 0xff61: return fail("j2k: PPT (packed packet headers) is not decoded");
      default: return true;  // COM, TLM, PLM, PLT, CRG and whatever else carries a length
    }
  };
  for (;;) {
    if (pos + 4 > n || d[pos] != 0xff) return fail("j2k: the main header ends without a tile-part");
    const uint32_t m = be16(d + pos);
    if (m == 0xff90) break;  // SOT
    L = seg_len(pos);
    if (L < 2 || pos + 2 + L > n) return fail("j2k: a marker segment runs beyond the file");
    if (!header_marker(m, d + pos + 4, L - 2, main, false)) return false;
    pos += 2 + L;
  }
  if (!main.have_cod || !main.have_qcd) return fail("j2k: the main header lacks COD or QCD");

  // ---- tile-parts: their bodies per tile, one after another
  struct TileData { Params P; std::vector<uint8_t> data; bool seen = false; int next_part = 0; };
  std::vector<TileData> tiles(ntiles);
  while (pos + 12 <= n && d[pos] == 0xff && d[pos + 1] == 0x90) {
    if (be16(d + pos + 2) != 10) return fail("j2k: SOT has another length than 10");
    const size_t isot = be16(d + pos + 4);
    uint64_t psot = be32(d + pos + 6);
    const int tpsot = d[pos + 10];
    if (isot >= ntiles) return fail("j2k: a tile-part of a tile the image lacks");
    if (psot == 0) psot = n - pos;
    if (psot < 14 || psot > n - pos) {
      if (psot < 14) return fail("j2k: a tile-part shorter than its header");
      psot = n - pos;  // a file cut short: what is there is decoded
    }
    TileData& T = tiles[isot];
    if (tpsot != T.next_part) return fail("j2k: the tile-parts of a tile out of order");
    ++T.next_part;
    if (!T.seen) { T.P = main; T.P.have_cod = false; T.seen = true; }
    ++f.tileparts;
    const size_t part_end = pos + (size_t)psot;
    size_t q = pos + 12;
    for (;;) {
      if (q + 2 > part_end || d[q] != 0xff) return fail("j2k: a tile-part header without SOD");
      const uint32_t m = be16(d + q);
      if (m == 0xff93) { q += 2; break; }  // SOD
      if (q + 4 > part_end) return fail("j2k: a tile-part header without SOD");
      L = be16(d + q + 2);
      if (L < 2 || q + 2 + L > part_end) return fail("j2k: a marker segment runs beyond its tile-part");
      if ((m == 0xff52 || m == 0xff5c) && tpsot != 0) return fail("j2k: COD or QCD in a later tile-part");
      if (!header_marker(m, d + q + 4, L - 2, T.P, true)) return false;
      q += 2 + L;
    }
    size_t body_end = part_end;
    if (part_end == n && body_end >= q + 2 && d[body_end - 2] == 0xff && d[body_end - 1] == 0xd9) body_end -= 2;  // EOC behind a Psot of 0
    T.data.insert(T.data.end(), d + q, d + body_end);
    pos = part_end;
  }
  // ---- colour
  if (!colours) colours = ncomps <= 2 ? 1 : 3;
  if (colours == 3 && ncomps < 3) colours = 1;
  int colour_comp[3] = {0, 1, 2};
  for (int k = 0; k < colours; ++k) {
    for (int i = 0; i < cdef_n; ++i)
      if (cdef[i][1] == 0 && cdef[i][2] == k + 1 && cdef[i][0] < ncomps) { colour_comp[k] = cdef[i][0]; break; }
  }
  for (size_t t = 0; t < ntiles; ++t)
    if (!tiles[t].seen) return fail("j2k: a tile without a tile-part");
  const Params& P0 = tiles[0].P;
  f.transform = P0.cod[0].transform;
  f.mct = P0.mct && ncomps >= 3;
  for (size_t t = 0; t < ntiles; ++t) {
    const Params& P = tiles[t].P;
    if ((P.mct && ncomps >= 3) != (f.mct != 0)) return fail("j2k: tiles that differ in their component transform are not decoded");
    for (int c = 0; c < ncomps; ++c)
      if (P.cod[c].transform != f.transform) return fail("j2k: components or tiles that differ in their wavelet transform are not decoded");
  }
  int carried[kMaxComps] = {-1, -1, -1, -1};
  if (f.mct) {
    f.ncomp = 3;
    carried[0] = 0; carried[1] = 1; carried[2] = 2;
    for (int k = 0; k < 3; ++k) f.chan[k] = colours == 3 ? colour_comp[k] : colour_comp[0];
    for (int k = 0; k < 3; ++k)
      if (f.chan[k] > 2) return fail("j2k: a colour channel outside the component transform");
  } else if (colours == 1) {
    f.ncomp = 1;
    carried[colour_comp[0]] = 0;
  } else {
    if (colour_comp[0] == colour_comp[1] || colour_comp[0] == colour_comp[2] || colour_comp[1] == colour_comp[2]) return fail("j2k: two colours in one component");
    f.ncomp = 3;
    for (int k = 0; k < 3; ++k) { carried[colour_comp[k]] = k; f.chan[k] = k; }
  }
  f.progression = P0.progression; f.layers = P0.layers; f.qstyle = P0.qnt[0].style; f.cbw = 1 << P0.cod[0].xcb; f.cbh = 1 << P0.cod[0].ycb;
  f.precincts = P0.cod[0].ppx[P0.cod[0].levels] != 15 || P0.cod[0].ppy[P0.cod[0].levels] != 15;
  f.sop = P0.sop; f.eph = P0.eph;
  // ---- tiles
  f.tcs.assign(ntiles * (size_t)f.ncomp, TileComp());
  for (size_t t = 0; t < ntiles; ++t) {
    const uint64_t p = t % tw, q = t / tw;
    Rect tile;
    tile.x0 = (int)std::max<uint64_t>(XTO + p * XT, XO); tile.y0 = (int)std::max<uint64_t>(YTO + q * YT, YO);
    tile.x1 = (int)std::min<uint64_t>(XTO + (p + 1) * XT, X); tile.y1 = (int)std::min<uint64_t>(YTO + (q + 1) * YT, Y);
    if (tile.x0 >= tile.x1 || tile.y0 >= tile.y1) return fail("j2k: an empty tile");
    if (!decode_tile(cd, tiles[t].P, ncomps, tile, tiles[t].data, carried, t * (size_t)f.ncomp, f.error)) return false;
    tiles[t].data = std::vector<uint8_t>();
  }
  if (const char* why = fault_of(f.width, f.height, f.x0, f.y0, f.ncomp, f.prec, f.transform, f.mct, f.chan, f.tcs.data(), f.tcs.size(), f.steps.size(), cd.ncoeffs))
    return fail(why);
  f.device_ok = device_fault(f.width, f.height, f.ncomp, f.tcs.data(), f.tcs.size()) == nullptr;
  return true;
}

// Tier-1 on the host: every block of `cd` into `coeffs` (cd.ncoeffs values, zeroed here).  false: the block list breaks a rule
// (coded_fault()).
inline bool tier1(const Coded& cd, int32_t* coeffs) {
  if (coded_fault(cd.frame.tcs.data(), cd.frame.tcs.size(), cd.cblks.data(), cd.cblks.size(), cd.bytes.size())) return false;
  std::fill(coeffs, coeffs + cd.ncoeffs, 0);
  detail::T1 t1;
  for (const CodedBlock& k : cd.cblks) {
    const TileComp& tc = cd.frame.tcs[k.tc];
    t1.run(cd.bytes.data() + k.byte_off, k.byte_len, k.numbps, k.passes, k.orient, k.w, k.h, coeffs + tc.coeff_off + k.at, (size_t)(tc.x1 - tc.x0));
  }
  return true;
}

// What parse_coded left to do, on this thread: `f` becomes cd's frame with its coefficients (cd gives its frame up).
inline bool finish_coded(Coded& cd, Frame& f) {
  std::vector<int32_t> coeffs(cd.ncoeffs);
  const bool ok = tier1(cd, coeffs.data());
  if (!ok) cd.frame.error = coded_fault(cd.frame.tcs.data(), cd.frame.tcs.size(), cd.cblks.data(), cd.cblks.size(), cd.bytes.size());
  f = std::move(cd.frame);
  if (ok) f.coeffs = std::move(coeffs);
  return ok;
}

// The serial half: parse_coded, then tier-1 on this thread.
inline bool parse(const uint8_t* d, size_t n, Frame& f) {
  Coded cd;
  if (!parse_coded(d, n, cd)) { f = std::move(cd.frame); return false; }
  return finish_coded(cd, f);
}

}  // namespace j2k
}  // namespace PaddleOCR
