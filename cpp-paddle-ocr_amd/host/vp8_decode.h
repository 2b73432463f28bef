// Lossy WebP (a VP8 key frame) decoder in two halves, shaped like webp_decode.h: whatever is serial on the caller's host
// thread - parse() - and the pixel part either on the device (csrc/kernels_vp8.hip, through ocr_vp8_frame) or here - pixels().
//
// What comes out is what cv::imdecode(data, IMREAD_COLOR) returns: the pixels of libwebp's WebPDecodeBGR (alpha dropped, no
// dithering, fancy upsampling, libwebp's fixed-point YUV -> RGB).  tests/test_vp8_decode.py compares with the system's libwebp.
//
// Container: webp::parse (webp_decode.h) walks the RIFF chunks and hands the "VP8 " payload over (Frame::vp8); an "ALPH" chunk
// in front of it is skipped, its content is not read.  parse_file() is that hand-over in one call.
//
// Serial half, parse(): the 3-byte frame tag (key frame, profile 0 .. 3, shown, first partition's length), start code
// 9d 01 2a, 14 bits of width and of height (the two scale bits on top of each are read and ignored, as libwebp ignores them);
// the boolean decoder; colour space and clamp bits (ignored); the segment header (quantiser and filter level per segment,
// absolute or delta, the three map probabilities); the filter header (simple / normal, level, sharpness, the ref and mode
// deltas); 1 / 2 / 4 / 8 token partitions (row y reads partition y & (n - 1); a partition size beyond the data is cut to it, the
// last partition must not be empty: libwebp's rules); the quantiser index with its five deltas; the coefficient probability
// updates and the skip probability; per macroblock the segment id, the skip flag, the luma mode (16x16 or B_PRED with the
// sub-block modes in the context of the modes above and to the left), the chroma mode; the token loop with its contexts.
// A read beyond a partition refuses the file where libwebp refuses it: after the header parts, after a row of modes, after
// a macroblock of tokens.  Inter frames, a frame that is not shown, a wrong start code, a zero dimension and a chunk
// shorter than its header are answered with kNoKeyFrame; what fails later is a bare decode failure.
//
// The frame descriptor (Frame; ocr_vp8_frame of include/ocr_hip.h states the same): one Mb record per macroblock in raster
// order - modes, filter parameters as libwebp's PrecomputeFilterStrengths and VP8DecodeMB make them (level 0 .. 63 after the
// segment and the deltas, interior limit, hev threshold, the "filter inner edges" flag), the 2-bit transform class of each of
// the 24 blocks and where its coefficients lie - and ONE array of dequantised coefficients that holds only the 4x4 blocks with
// a non-zero entry, 16 int16 each in raster (not zigzag) order: Mb::present has bit b set when block b is shipped (0 .. 15 luma
// in raster order, 16 .. 19 U, 20 .. 23 V, 24 the Y2 block of a 16x16-predicted macroblock), and block b is the
// popcount(present & ((1 << b) - 1))-th block behind Mb::coeff_off.  A coefficient is libwebp's: (int16_t)(value * quantiser),
// wrap included.  The luma blocks of a macroblock with a Y2 block carry 0 as their DC: the inverse WHT (pixels()) makes it.
//
// Pixel half, pixels(), and kernels_vp8.hip after it:
//   - inverse WHT of the Y2 block (outputs stored as int16_t, as libwebp stores them) into the DC of the 16 luma blocks
//   - per block the inverse DCT libwebp runs for its class: 3 (a token beyond the third position) the full transform, 2 the
//     three-coefficient form, else the DC form when the DC is not zero.  In exact arithmetic the three agree; for products
//     that wrapped they do not, because libwebp's full transform (its SSE2 form) works in wrapping 16-bit lanes where the two
//     short forms work in int.  The installed libwebp is the yardstick, so the three are kept apart, and a chroma plane with
//     any class >= 2 takes the full transform for all four blocks, as libwebp's DoUVTransform does
//   - intra prediction from UNFILTERED neighbours; above the frame 127, left of it 129, the corner above-left 127 on the top
//     row and 129 below it; DC prediction without the missing side(s); a B_PRED macroblock's sub-blocks in raster order, the
//     four pixels above-right of the macroblock (those of the macroblock above-right; the last pixel above replicated in the
//     last column; 127 on the top row) also serve rows 1 .. 3 of its right-most sub-blocks
//   - the loop filter over the whole frame in macroblock raster order: left edge, inner vertical edges, top edge, inner
//     horizontal edges; no frame-left and frame-top edge; inner edges only where the flag is set; level 0 filters nothing;
//     simple (luma only) or normal
//   - crop to width x height, fancy upsampling of U and V (9-3-3-1), BGR by libwebp's 14-bit fixed point
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "webp_decode.h"

// the pixel half's arithmetic is stated once: csrc/kernels_vp8.hip compiles these functions for the device too
#ifdef __HIPCC__
#define VP8_FN __host__ __device__ inline
#else
#define VP8_FN inline
#endif

namespace PaddleOCR {
namespace vp8 {

// what a VP8 chunk without a decodable key-frame header is answered with (the text in front of the parenthesis is
// webp::kNotLossless's: one reply for everything that is not a still image this service decodes)
constexpr const char* kNoKeyFrame = "lossy or animated WebP is not decoded (the VP8 chunk holds no key-frame header)";

enum { DC_PRED = 0, TM_PRED = 1, V_PRED = 2, H_PRED = 3 };  // 16x16 luma and chroma; the first four sub-block modes too
enum { B_DC = 0, B_TM, B_VE, B_HE, B_RD, B_VR, B_LD, B_VL, B_HD, B_HU, kBModes };

struct Mb {  // ocr_vp8_mb of include/ocr_hip.h, field for field
  uint8_t modes[16];   // is_i4x4: the sub-block modes in raster order; else modes[0] is the 16x16 mode
  uint8_t is_i4x4, uvmode;
  uint8_t level, ilevel, hev, inner;  // loop filter: level 0 .. 63 (0: none), interior limit, hev threshold, inner edges too
  uint8_t segment, skip;              // as coded (informative: the pixel half does not read them)
  uint32_t nz_y, nz_uv;               // 2 bits a block, libwebp's order: luma block 0 in bits 31 .. 30; U block 0 in 7 .. 6, V in 15 .. 14
  uint32_t present, coeff_off;        // see the head of the file; coeff_off counts blocks of 16
};
static_assert(sizeof(Mb) == 40, "Mb is part of the C ABI");

struct Frame {
  int width = 0, height = 0;
  int filter_type = 0;           // 0 none, 1 simple, 2 normal
  std::vector<Mb> mbs;           // mb_w(frame) * mb_h(frame)
  std::vector<int16_t> coeffs;   // 16 per shipped block
  int partitions = 0, segments = 0;  // informative: token partitions; 4 when the segment map is coded, else 1
  const char* error = nullptr;   // why parse() refused (nullptr: a bare decode failure)
};
inline int mb_w(const Frame& f) { return (f.width + 15) >> 4; }
inline int mb_h(const Frame& f) { return (f.height + 15) >> 4; }

// why pixels() (and the device stage, which states the same rules over ocr_vp8_frame) refuses a frame; nullptr when sound
inline const char* fault_of(int width, int height, int filter_type, const Mb* mbs, size_t nmbs, size_t ncoeffs) {
  if (width < 1 || height < 1 || width > 16383 || height > 16383) return "vp8 frame: width and height must be 1 .. 16383";
  if (filter_type < 0 || filter_type > 2) return "vp8 frame: filter type must be 0 .. 2";
  const size_t need = (size_t)((width + 15) >> 4) * ((height + 15) >> 4);
  if (!mbs || nmbs < need) return "vp8 frame: fewer macroblock records than the frame has macroblocks";
  for (size_t i = 0; i < need; ++i) {
    const Mb& m = mbs[i];
    if (m.is_i4x4 > 1) return "vp8 frame: is_i4x4 must be 0 or 1";
    if (m.uvmode > H_PRED) return "vp8 frame: chroma mode must be 0 .. 3";
    if (m.is_i4x4) {
      for (int k = 0; k < 16; ++k)
        if (m.modes[k] >= kBModes) return "vp8 frame: sub-block mode must be 0 .. 9";
    } else if (m.modes[0] > H_PRED) {
      return "vp8 frame: 16x16 mode must be 0 .. 3";
    }
    if (m.level > 63) return "vp8 frame: filter level must be 0 .. 63";
    if (m.ilevel > 63 || m.hev > 2 || m.inner > 1) return "vp8 frame: interior limit 0 .. 63, hev threshold 0 .. 2, inner flag 0 or 1";
    if (m.present >> 25) return "vp8 frame: a macroblock has 25 blocks";
    if (m.is_i4x4 && (m.present >> 24)) return "vp8 frame: a B_PRED macroblock has no Y2 block";
    if (m.nz_uv >> 16) return "vp8 frame: chroma classes take 16 bits";
    if ((size_t)m.coeff_off + (size_t)__builtin_popcount(m.present) > ncoeffs / 16) return "vp8 frame: a macroblock's coefficients lie beyond the array";
  }
  return nullptr;
}
inline const char* fault(const Frame& f) { return fault_of(f.width, f.height, f.filter_type, f.mbs.data(), f.mbs.size(), f.coeffs.size()); }

// ---------------------------------------------------------------------------------------------------------------- tables
namespace detail {

// The format's constants as the installed libwebp holds them: default coefficient probabilities [type][band][context][node],
// the probabilities of their updates, sub-block mode probabilities [mode above][mode left][node], the quantiser tables.
constexpr uint8_t kCoeffProba0[1056] = {
    128, 128, 128, 128, 128, 128, 128, 128, 128, 128, 128, 128, 128, 128, 128, 128, 128, 128, 128, 128, 128, 128,
    128, 128, 128, 128, 128, 128, 128, 128, 128, 128, 128, 253, 136, 254, 255, 228, 219, 128, 128, 128, 128, 128,
    189, 129, 242, 255, 227, 213, 255, 219, 128, 128, 128, 106, 126, 227, 252, 214, 209, 255, 255, 128, 128, 128,
    1, 98, 248, 255, 236, 226, 255, 255, 128, 128, 128, 181, 133, 238, 254, 221, 234, 255, 154, 128, 128, 128,
    78, 134, 202, 247, 198, 180, 255, 219, 128, 128, 128, 1, 185, 249, 255, 243, 255, 128, 128, 128, 128, 128,
    184, 150, 247, 255, 236, 224, 128, 128, 128, 128, 128, 77, 110, 216, 255, 236, 230, 128, 128, 128, 128, 128,
    1, 101, 251, 255, 241, 255, 128, 128, 128, 128, 128, 170, 139, 241, 252, 236, 209, 255, 255, 128, 128, 128,
    37, 116, 196, 243, 228, 255, 255, 255, 128, 128, 128, 1, 204, 254, 255, 245, 255, 128, 128, 128, 128, 128,
    207, 160, 250, 255, 238, 128, 128, 128, 128, 128, 128, 102, 103, 231, 255, 211, 171, 128, 128, 128, 128, 128,
    1, 152, 252, 255, 240, 255, 128, 128, 128, 128, 128, 177, 135, 243, 255, 234, 225, 128, 128, 128, 128, 128,
    80, 129, 211, 255, 194, 224, 128, 128, 128, 128, 128, 1, 1, 255, 128, 128, 128, 128, 128, 128, 128, 128,
    246, 1, 255, 128, 128, 128, 128, 128, 128, 128, 128, 255, 128, 128, 128, 128, 128, 128, 128, 128, 128, 128,
    198, 35, 237, 223, 193, 187, 162, 160, 145, 155, 62, 131, 45, 198, 221, 172, 176, 220, 157, 252, 221, 1,
    68, 47, 146, 208, 149, 167, 221, 162, 255, 223, 128, 1, 149, 241, 255, 221, 224, 255, 255, 128, 128, 128,
    184, 141, 234, 253, 222, 220, 255, 199, 128, 128, 128, 81, 99, 181, 242, 176, 190, 249, 202, 255, 255, 128,
    1, 129, 232, 253, 214, 197, 242, 196, 255, 255, 128, 99, 121, 210, 250, 201, 198, 255, 202, 128, 128, 128,
    23, 91, 163, 242, 170, 187, 247, 210, 255, 255, 128, 1, 200, 246, 255, 234, 255, 128, 128, 128, 128, 128,
    109, 178, 241, 255, 231, 245, 255, 255, 128, 128, 128, 44, 130, 201, 253, 205, 192, 255, 255, 128, 128, 128,
    1, 132, 239, 251, 219, 209, 255, 165, 128, 128, 128, 94, 136, 225, 251, 218, 190, 255, 255, 128, 128, 128,
    22, 100, 174, 245, 186, 161, 255, 199, 128, 128, 128, 1, 182, 249, 255, 232, 235, 128, 128, 128, 128, 128,
    124, 143, 241, 255, 227, 234, 128, 128, 128, 128, 128, 35, 77, 181, 251, 193, 211, 255, 205, 128, 128, 128,
    1, 157, 247, 255, 236, 231, 255, 255, 128, 128, 128, 121, 141, 235, 255, 225, 227, 255, 255, 128, 128, 128,
    45, 99, 188, 251, 195, 217, 255, 224, 128, 128, 128, 1, 1, 251, 255, 213, 255, 128, 128, 128, 128, 128,
    203, 1, 248, 255, 255, 128, 128, 128, 128, 128, 128, 137, 1, 177, 255, 224, 255, 128, 128, 128, 128, 128,
    253, 9, 248, 251, 207, 208, 255, 192, 128, 128, 128, 175, 13, 224, 243, 193, 185, 249, 198, 255, 255, 128,
    73, 17, 171, 221, 161, 179, 236, 167, 255, 234, 128, 1, 95, 247, 253, 212, 183, 255, 255, 128, 128, 128,
    239, 90, 244, 250, 211, 209, 255, 255, 128, 128, 128, 155, 77, 195, 248, 188, 195, 255, 255, 128, 128, 128,
    1, 24, 239, 251, 218, 219, 255, 205, 128, 128, 128, 201, 51, 219, 255, 196, 186, 128, 128, 128, 128, 128,
    69, 46, 190, 239, 201, 218, 255, 228, 128, 128, 128, 1, 191, 251, 255, 255, 128, 128, 128, 128, 128, 128,
    223, 165, 249, 255, 213, 255, 128, 128, 128, 128, 128, 141, 124, 248, 255, 255, 128, 128, 128, 128, 128, 128,
    1, 16, 248, 255, 255, 128, 128, 128, 128, 128, 128, 190, 36, 230, 255, 236, 255, 128, 128, 128, 128, 128,
    149, 1, 255, 128, 128, 128, 128, 128, 128, 128, 128, 1, 226, 255, 128, 128, 128, 128, 128, 128, 128, 128,
    247, 192, 255, 128, 128, 128, 128, 128, 128, 128, 128, 240, 128, 255, 128, 128, 128, 128, 128, 128, 128, 128,
    1, 134, 252, 255, 255, 128, 128, 128, 128, 128, 128, 213, 62, 250, 255, 255, 128, 128, 128, 128, 128, 128,
    55, 93, 255, 128, 128, 128, 128, 128, 128, 128, 128, 128, 128, 128, 128, 128, 128, 128, 128, 128, 128, 128,
    128, 128, 128, 128, 128, 128, 128, 128, 128, 128, 128, 128, 128, 128, 128, 128, 128, 128, 128, 128, 128, 128,
    202, 24, 213, 235, 186, 191, 220, 160, 240, 175, 255, 126, 38, 182, 232, 169, 184, 228, 174, 255, 187, 128,
    61, 46, 138, 219, 151, 178, 240, 170, 255, 216, 128, 1, 112, 230, 250, 199, 191, 247, 159, 255, 255, 128,
    166, 109, 228, 252, 211, 215, 255, 174, 128, 128, 128, 39, 77, 162, 232, 172, 180, 245, 178, 255, 255, 128,
    1, 52, 220, 246, 198, 199, 249, 220, 255, 255, 128, 124, 74, 191, 243, 183, 193, 250, 221, 255, 255, 128,
    24, 71, 130, 219, 154, 170, 243, 182, 255, 255, 128, 1, 182, 225, 249, 219, 240, 255, 224, 128, 128, 128,
    149, 150, 226, 252, 216, 205, 255, 171, 128, 128, 128, 28, 108, 170, 242, 183, 194, 254, 223, 255, 255, 128,
    1, 81, 230, 252, 204, 203, 255, 192, 128, 128, 128, 123, 102, 209, 247, 188, 196, 255, 233, 128, 128, 128,
    20, 95, 153, 243, 164, 173, 255, 203, 128, 128, 128, 1, 222, 248, 255, 216, 213, 128, 128, 128, 128, 128,
    168, 175, 246, 252, 235, 205, 255, 255, 128, 128, 128, 47, 116, 215, 255, 211, 212, 255, 255, 128, 128, 128,
    1, 121, 236, 253, 212, 214, 255, 255, 128, 128, 128, 141, 84, 213, 252, 201, 202, 255, 219, 128, 128, 128,
    42, 80, 160, 240, 162, 185, 255, 205, 128, 128, 128, 1, 1, 255, 128, 128, 128, 128, 128, 128, 128, 128,
    244, 1, 255, 128, 128, 128, 128, 128, 128, 128, 128, 238, 1, 255, 128, 128, 128, 128, 128, 128, 128, 128};
constexpr uint8_t kCoeffUpdateProba[1056] = {
    255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255,
    255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 176, 246, 255, 255, 255, 255, 255, 255, 255, 255, 255,
    223, 241, 252, 255, 255, 255, 255, 255, 255, 255, 255, 249, 253, 253, 255, 255, 255, 255, 255, 255, 255, 255,
    255, 244, 252, 255, 255, 255, 255, 255, 255, 255, 255, 234, 254, 254, 255, 255, 255, 255, 255, 255, 255, 255,
    253, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 246, 254, 255, 255, 255, 255, 255, 255, 255, 255,
    239, 253, 254, 255, 255, 255, 255, 255, 255, 255, 255, 254, 255, 254, 255, 255, 255, 255, 255, 255, 255, 255,
    255, 248, 254, 255, 255, 255, 255, 255, 255, 255, 255, 251, 255, 254, 255, 255, 255, 255, 255, 255, 255, 255,
    255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 253, 254, 255, 255, 255, 255, 255, 255, 255, 255,
    251, 254, 254, 255, 255, 255, 255, 255, 255, 255, 255, 254, 255, 254, 255, 255, 255, 255, 255, 255, 255, 255,
    255, 254, 253, 255, 254, 255, 255, 255, 255, 255, 255, 250, 255, 254, 255, 254, 255, 255, 255, 255, 255, 255,
    254, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255,
    255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255,
    217, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 225, 252, 241, 253, 255, 255, 254, 255, 255, 255, 255,
    234, 250, 241, 250, 253, 255, 253, 254, 255, 255, 255, 255, 254, 255, 255, 255, 255, 255, 255, 255, 255, 255,
    223, 254, 254, 255, 255, 255, 255, 255, 255, 255, 255, 238, 253, 254, 254, 255, 255, 255, 255, 255, 255, 255,
    255, 248, 254, 255, 255, 255, 255, 255, 255, 255, 255, 249, 254, 255, 255, 255, 255, 255, 255, 255, 255, 255,
    255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 253, 255, 255, 255, 255, 255, 255, 255, 255, 255,
    247, 254, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255,
    255, 253, 254, 255, 255, 255, 255, 255, 255, 255, 255, 252, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255,
    255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 254, 254, 255, 255, 255, 255, 255, 255, 255, 255,
    253, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255,
    255, 254, 253, 255, 255, 255, 255, 255, 255, 255, 255, 250, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255,
    254, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255,
    255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255,
    186, 251, 250, 255, 255, 255, 255, 255, 255, 255, 255, 234, 251, 244, 254, 255, 255, 255, 255, 255, 255, 255,
    251, 251, 243, 253, 254, 255, 254, 255, 255, 255, 255, 255, 253, 254, 255, 255, 255, 255, 255, 255, 255, 255,
    236, 253, 254, 255, 255, 255, 255, 255, 255, 255, 255, 251, 253, 253, 254, 254, 255, 255, 255, 255, 255, 255,
    255, 254, 254, 255, 255, 255, 255, 255, 255, 255, 255, 254, 254, 254, 255, 255, 255, 255, 255, 255, 255, 255,
    255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 254, 255, 255, 255, 255, 255, 255, 255, 255, 255,
    254, 254, 255, 255, 255, 255, 255, 255, 255, 255, 255, 254, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255,
    255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 254, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255,
    255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255,
    255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255,
    255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255,
    255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255,
    255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255,
    248, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 250, 254, 252, 254, 255, 255, 255, 255, 255, 255, 255,
    248, 254, 249, 253, 255, 255, 255, 255, 255, 255, 255, 255, 253, 253, 255, 255, 255, 255, 255, 255, 255, 255,
    246, 253, 253, 255, 255, 255, 255, 255, 255, 255, 255, 252, 254, 251, 254, 254, 255, 255, 255, 255, 255, 255,
    255, 254, 252, 255, 255, 255, 255, 255, 255, 255, 255, 248, 254, 253, 255, 255, 255, 255, 255, 255, 255, 255,
    253, 255, 254, 254, 255, 255, 255, 255, 255, 255, 255, 255, 251, 254, 255, 255, 255, 255, 255, 255, 255, 255,
    245, 251, 254, 255, 255, 255, 255, 255, 255, 255, 255, 253, 253, 254, 255, 255, 255, 255, 255, 255, 255, 255,
    255, 251, 253, 255, 255, 255, 255, 255, 255, 255, 255, 252, 253, 254, 255, 255, 255, 255, 255, 255, 255, 255,
    255, 254, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 252, 255, 255, 255, 255, 255, 255, 255, 255, 255,
    249, 255, 254, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 254, 255, 255, 255, 255, 255, 255, 255, 255,
    255, 255, 253, 255, 255, 255, 255, 255, 255, 255, 255, 250, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255,
    255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255,
    254, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255};
constexpr uint8_t kBModesProba[900] = {
    231, 120, 48, 89, 115, 113, 120, 152, 112, 152, 179, 64, 126, 170, 118, 46, 70, 95,
    175, 69, 143, 80, 85, 82, 72, 155, 103, 56, 58, 10, 171, 218, 189, 17, 13, 152,
    114, 26, 17, 163, 44, 195, 21, 10, 173, 121, 24, 80, 195, 26, 62, 44, 64, 85,
    144, 71, 10, 38, 171, 213, 144, 34, 26, 170, 46, 55, 19, 136, 160, 33, 206, 71,
    63, 20, 8, 114, 114, 208, 12, 9, 226, 81, 40, 11, 96, 182, 84, 29, 16, 36,
    134, 183, 89, 137, 98, 101, 106, 165, 148, 72, 187, 100, 130, 157, 111, 32, 75, 80,
    66, 102, 167, 99, 74, 62, 40, 234, 128, 41, 53, 9, 178, 241, 141, 26, 8, 107,
    74, 43, 26, 146, 73, 166, 49, 23, 157, 65, 38, 105, 160, 51, 52, 31, 115, 128,
    104, 79, 12, 27, 217, 255, 87, 17, 7, 87, 68, 71, 44, 114, 51, 15, 186, 23,
    47, 41, 14, 110, 182, 183, 21, 17, 194, 66, 45, 25, 102, 197, 189, 23, 18, 22,
    88, 88, 147, 150, 42, 46, 45, 196, 205, 43, 97, 183, 117, 85, 38, 35, 179, 61,
    39, 53, 200, 87, 26, 21, 43, 232, 171, 56, 34, 51, 104, 114, 102, 29, 93, 77,
    39, 28, 85, 171, 58, 165, 90, 98, 64, 34, 22, 116, 206, 23, 34, 43, 166, 73,
    107, 54, 32, 26, 51, 1, 81, 43, 31, 68, 25, 106, 22, 64, 171, 36, 225, 114,
    34, 19, 21, 102, 132, 188, 16, 76, 124, 62, 18, 78, 95, 85, 57, 50, 48, 51,
    193, 101, 35, 159, 215, 111, 89, 46, 111, 60, 148, 31, 172, 219, 228, 21, 18, 111,
    112, 113, 77, 85, 179, 255, 38, 120, 114, 40, 42, 1, 196, 245, 209, 10, 25, 109,
    88, 43, 29, 140, 166, 213, 37, 43, 154, 61, 63, 30, 155, 67, 45, 68, 1, 209,
    100, 80, 8, 43, 154, 1, 51, 26, 71, 142, 78, 78, 16, 255, 128, 34, 197, 171,
    41, 40, 5, 102, 211, 183, 4, 1, 221, 51, 50, 17, 168, 209, 192, 23, 25, 82,
    138, 31, 36, 171, 27, 166, 38, 44, 229, 67, 87, 58, 169, 82, 115, 26, 59, 179,
    63, 59, 90, 180, 59, 166, 93, 73, 154, 40, 40, 21, 116, 143, 209, 34, 39, 175,
    47, 15, 16, 183, 34, 223, 49, 45, 183, 46, 17, 33, 183, 6, 98, 15, 32, 183,
    57, 46, 22, 24, 128, 1, 54, 17, 37, 65, 32, 73, 115, 28, 128, 23, 128, 205,
    40, 3, 9, 115, 51, 192, 18, 6, 223, 87, 37, 9, 115, 59, 77, 64, 21, 47,
    104, 55, 44, 218, 9, 54, 53, 130, 226, 64, 90, 70, 205, 40, 41, 23, 26, 57,
    54, 57, 112, 184, 5, 41, 38, 166, 213, 30, 34, 26, 133, 152, 116, 10, 32, 134,
    39, 19, 53, 221, 26, 114, 32, 73, 255, 31, 9, 65, 234, 2, 15, 1, 118, 73,
    75, 32, 12, 51, 192, 255, 160, 43, 51, 88, 31, 35, 67, 102, 85, 55, 186, 85,
    56, 21, 23, 111, 59, 205, 45, 37, 192, 55, 38, 70, 124, 73, 102, 1, 34, 98,
    125, 98, 42, 88, 104, 85, 117, 175, 82, 95, 84, 53, 89, 128, 100, 113, 101, 45,
    75, 79, 123, 47, 51, 128, 81, 171, 1, 57, 17, 5, 71, 102, 57, 53, 41, 49,
    38, 33, 13, 121, 57, 73, 26, 1, 85, 41, 10, 67, 138, 77, 110, 90, 47, 114,
    115, 21, 2, 10, 102, 255, 166, 23, 6, 101, 29, 16, 10, 85, 128, 101, 196, 26,
    57, 18, 10, 102, 102, 213, 34, 20, 43, 117, 20, 15, 36, 163, 128, 68, 1, 26,
    102, 61, 71, 37, 34, 53, 31, 243, 192, 69, 60, 71, 38, 73, 119, 28, 222, 37,
    68, 45, 128, 34, 1, 47, 11, 245, 171, 62, 17, 19, 70, 146, 85, 55, 62, 70,
    37, 43, 37, 154, 100, 163, 85, 160, 1, 63, 9, 92, 136, 28, 64, 32, 201, 85,
    75, 15, 9, 9, 64, 255, 184, 119, 16, 86, 6, 28, 5, 64, 255, 25, 248, 1,
    56, 8, 17, 132, 137, 255, 55, 116, 128, 58, 15, 20, 82, 135, 57, 26, 121, 40,
    164, 50, 31, 137, 154, 133, 25, 35, 218, 51, 103, 44, 131, 131, 123, 31, 6, 158,
    86, 40, 64, 135, 148, 224, 45, 183, 128, 22, 26, 17, 131, 240, 154, 14, 1, 209,
    45, 16, 21, 91, 64, 222, 7, 1, 197, 56, 21, 39, 155, 60, 138, 23, 102, 213,
    83, 12, 13, 54, 192, 255, 68, 47, 28, 85, 26, 85, 85, 128, 128, 32, 146, 171,
    18, 11, 7, 63, 144, 171, 4, 4, 246, 35, 27, 10, 146, 174, 171, 12, 26, 128,
    190, 80, 35, 99, 180, 80, 126, 54, 45, 85, 126, 47, 87, 176, 51, 41, 20, 32,
    101, 75, 128, 139, 118, 146, 116, 128, 85, 56, 41, 15, 176, 236, 85, 37, 9, 62,
    71, 30, 17, 119, 118, 255, 17, 18, 138, 101, 38, 60, 138, 55, 70, 43, 26, 142,
    146, 36, 19, 30, 171, 255, 97, 27, 20, 138, 45, 61, 62, 219, 1, 81, 188, 64,
    32, 41, 20, 117, 151, 142, 20, 21, 163, 112, 19, 12, 61, 195, 128, 48, 4, 24};
constexpr uint8_t kDcTable[128] = {
    4, 5, 6, 7, 8, 9, 10, 10, 11, 12, 13, 14, 15, 16, 17, 17, 18, 19, 20, 20, 21, 21, 22, 22, 23, 23, 24, 25, 25, 26, 27, 28,
    29, 30, 31, 32, 33, 34, 35, 36, 37, 37, 38, 39, 40, 41, 42, 43, 44, 45, 46, 46, 47, 48, 49, 50, 51, 52, 53, 54, 55, 56, 57, 58,
    59, 60, 61, 62, 63, 64, 65, 66, 67, 68, 69, 70, 71, 72, 73, 74, 75, 76, 76, 77, 78, 79, 80, 81, 82, 83, 84, 85, 86, 87, 88, 89,
    91, 93, 95, 96, 98, 100, 101, 102, 104, 106, 108, 110, 112, 114, 116, 118, 122, 124, 126, 128, 130, 132, 134, 136, 138, 140, 143, 145, 148, 151, 154, 157};
constexpr uint16_t kAcTable[128] = {
    4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23, 24, 25, 26, 27,
    28, 29, 30, 31, 32, 33, 34, 35, 36, 37, 38, 39, 40, 41, 42, 43, 44, 45, 46, 47, 48, 49, 50, 51,
    52, 53, 54, 55, 56, 57, 58, 60, 62, 64, 66, 68, 70, 72, 74, 76, 78, 80, 82, 84, 86, 88, 90, 92,
    94, 96, 98, 100, 102, 104, 106, 108, 110, 112, 114, 116, 119, 122, 125, 128, 131, 134, 137, 140, 143, 146, 149, 152,
    155, 158, 161, 164, 167, 170, 173, 177, 181, 185, 189, 193, 197, 201, 205, 209, 213, 217, 221, 225, 229, 234, 239, 245,
    249, 254, 259, 264, 269, 274, 279, 284};
constexpr uint8_t kZigzag[16] = {0, 1, 4, 8, 5, 2, 3, 6, 9, 12, 13, 10, 7, 11, 14, 15};
constexpr uint8_t kBands[17] = {0, 1, 2, 3, 6, 4, 5, 6, 6, 6, 6, 6, 6, 6, 6, 7, 0};  // [16]: what follows the last coefficient
constexpr uint8_t kCat3[] = {173, 148, 140, 0}, kCat4[] = {176, 155, 140, 135, 0}, kCat5[] = {180, 157, 141, 134, 130, 0},
                  kCat6[] = {254, 254, 243, 230, 196, 177, 153, 140, 133, 130, 129, 0};
// the sub-block mode tree: a positive entry is the next pair, a non-positive one minus a mode
constexpr int8_t kBModeTree[18] = {-B_DC, 1, -B_TM, 2, -B_VE, 3, 4, 6, -B_HE, 5, -B_RD, -B_VR, -B_LD, 7, -B_VL, 8, -B_HD, -B_HU};
inline const uint8_t* coeff_proba0(int t, int b, int c) { return kCoeffProba0 + ((t * 8 + b) * 3 + c) * 11; }

// the boolean decoder.  Past the end of its bytes it reads eight zero bits once and raises eof, as libwebp's does
struct Bool {
  const uint8_t *p, *end;
  uint32_t value = 0, range = 255;
  int bits = -8;
  bool eof = false;
  Bool() : p(nullptr), end(nullptr) {}
  Bool(const uint8_t* d, size_t n) : p(d), end(d + n) {}
  void load() {
    if (p < end) { value = (value << 8) | *p++; bits += 8; }
    else if (!eof) { value <<= 8; bits += 8; eof = true; }
    else bits = 0;
  }
  int get(int prob) {
    if (bits < 0) load();
    const uint32_t split = 1 + (((range - 1) * (uint32_t)prob) >> 8);
    const int bit = (value >> bits) >= split;
    if (bit) { range -= split; value -= split << bits; }
    else range = split;
    while (range < 128) { range <<= 1; --bits; }
    return bit;
  }
  int bit() { return get(128); }
  int literal(int n) {
    int v = 0;
    while (n-- > 0) v |= bit() << n;
    return v;
  }
  int sliteral(int n) {
    const int v = literal(n);
    return bit() ? -v : v;
  }
};

VP8_FN int clip(int v, int hi) { return v < 0 ? 0 : v > hi ? hi : v; }
VP8_FN uint8_t clip8(int v) { return (uint8_t)(v < 0 ? 0 : v > 255 ? 255 : v); }

// the inverse WHT of the Y2 block: out[step * k] is the DC of luma block k
VP8_FN void wht(const int16_t* in, int16_t* out, int step = 16) {
  int tmp[16];
  for (int i = 0; i < 4; ++i) {
    const int a0 = in[0 + i] + in[12 + i], a1 = in[4 + i] + in[8 + i], a2 = in[4 + i] - in[8 + i], a3 = in[0 + i] - in[12 + i];
    tmp[0 + i] = a0 + a1; tmp[8 + i] = a0 - a1; tmp[4 + i] = a3 + a2; tmp[12 + i] = a3 - a2;
  }
  for (int i = 0; i < 4; ++i) {
    const int dc = tmp[0 + i * 4] + 3;
    const int a0 = dc + tmp[3 + i * 4], a1 = tmp[1 + i * 4] + tmp[2 + i * 4], a2 = tmp[1 + i * 4] - tmp[2 + i * 4], a3 = dc - tmp[3 + i * 4];
    out[0] = (int16_t)((a0 + a1) >> 3); out[step] = (int16_t)((a3 + a2) >> 3); out[2 * step] = (int16_t)((a0 - a1) >> 3); out[3 * step] = (int16_t)((a3 - a2) >> 3);
    out += 4 * step;
  }
}

struct Parser {
  Bool br;          // the first partition
  Bool part[8];
  int nparts = 1;
  // headers
  int use_segment = 0, update_map = 0, absolute_delta = 1;
  int quantizer[4] = {}, filter_strength[4] = {};
  uint8_t segment_proba[3] = {255, 255, 255};
  int simple = 0, level = 0, sharpness = 0, use_lf_delta = 0, ref_lf_delta[4] = {}, mode_lf_delta[4] = {};
  int y1[4][2], y2[4][2], uv[4][2];
  uint8_t proba[4][8][3][11];
  int use_skip = 0, skip_p = 0;
  struct Strength { uint8_t level, ilevel, hev, inner; } strength[4][2] = {};

  bool segment_header() {
    use_segment = br.bit();
    if (use_segment) {
      update_map = br.bit();
      if (br.bit()) {
        absolute_delta = br.bit();
        for (int s = 0; s < 4; ++s) quantizer[s] = br.bit() ? br.sliteral(7) : 0;
        for (int s = 0; s < 4; ++s) filter_strength[s] = br.bit() ? br.sliteral(6) : 0;
      }
      if (update_map)
        for (int s = 0; s < 3; ++s) segment_proba[s] = br.bit() ? (uint8_t)br.literal(8) : 255;
    } else {
      update_map = 0;
    }
    return !br.eof;
  }
  bool filter_header() {
    simple = br.bit();
    level = br.literal(6);
    sharpness = br.literal(3);
    use_lf_delta = br.bit();
    if (use_lf_delta && br.bit()) {
      for (int i = 0; i < 4; ++i) if (br.bit()) ref_lf_delta[i] = br.sliteral(6);
      for (int i = 0; i < 4; ++i) if (br.bit()) mode_lf_delta[i] = br.sliteral(6);
    }
    return !br.eof;
  }
  void quant() {
    const int base = br.literal(7);
    const int dqy1_dc = br.bit() ? br.sliteral(4) : 0, dqy2_dc = br.bit() ? br.sliteral(4) : 0, dqy2_ac = br.bit() ? br.sliteral(4) : 0;
    const int dquv_dc = br.bit() ? br.sliteral(4) : 0, dquv_ac = br.bit() ? br.sliteral(4) : 0;
    for (int i = 0; i < 4; ++i) {
      int q = base;
      if (use_segment) q = quantizer[i] + (absolute_delta ? 0 : base);
      y1[i][0] = kDcTable[clip(q + dqy1_dc, 127)];
      y1[i][1] = kAcTable[clip(q, 127)];
      y2[i][0] = kDcTable[clip(q + dqy2_dc, 127)] * 2;
      y2[i][1] = (kAcTable[clip(q + dqy2_ac, 127)] * 101581) >> 16;  // x * 155 / 100
      if (y2[i][1] < 8) y2[i][1] = 8;
      uv[i][0] = kDcTable[clip(q + dquv_dc, 117)];
      uv[i][1] = kAcTable[clip(q + dquv_ac, 127)];
    }
  }
  void probas() {
    for (int t = 0; t < 4; ++t)
      for (int b = 0; b < 8; ++b)
        for (int c = 0; c < 3; ++c)
          for (int p = 0; p < 11; ++p) {
            const int at = ((t * 8 + b) * 3 + c) * 11 + p;
            proba[t][b][c][p] = br.get(kCoeffUpdateProba[at]) ? (uint8_t)br.literal(8) : kCoeffProba0[at];
          }
    use_skip = br.bit();
    if (use_skip) skip_p = br.literal(8);
  }
  void strengths(int filter_type) {
    if (!filter_type) return;
    for (int s = 0; s < 4; ++s) {
      int base_level = level;
      if (use_segment) base_level = filter_strength[s] + (absolute_delta ? 0 : level);
      for (int i4 = 0; i4 <= 1; ++i4) {
        Strength& info = strength[s][i4];
        int lv = base_level;
        if (use_lf_delta) {
          lv += ref_lf_delta[0];
          if (i4) lv += mode_lf_delta[0];
        }
        lv = clip(lv, 63);
        info = Strength{0, 0, 0, (uint8_t)i4};
        if (lv > 0) {
          int il = lv;
          if (sharpness > 0) {
            il >>= sharpness > 4 ? 2 : 1;
            if (il > 9 - sharpness) il = 9 - sharpness;
          }
          if (il < 1) il = 1;
          info.level = (uint8_t)lv;
          info.ilevel = (uint8_t)il;
          info.hev = lv >= 40 ? 2 : lv >= 15 ? 1 : 0;
        }
      }
    }
  }

  int large_value(Bool& b, const uint8_t* p) {
    if (!b.get(p[3])) return !b.get(p[4]) ? 2 : 3 + b.get(p[5]);
    if (!b.get(p[6])) {
      if (!b.get(p[7])) return 5 + b.get(159);
      const int v = 7 + 2 * b.get(165);
      return v + b.get(145);
    }
    const int bit1 = b.get(p[8]), bit0 = b.get(p[9 + bit1]), cat = 2 * bit1 + bit0;
    const uint8_t* tab = cat == 0 ? kCat3 : cat == 1 ? kCat4 : cat == 2 ? kCat5 : kCat6;
    int v = 0;
    for (; *tab; ++tab) v += v + b.get(*tab);
    return v + 3 + (8 << cat);
  }
  // the tokens of one block of type t from position n on; the position behind the last token
  int block(Bool& b, int t, int ctx, const int* dq, int n, int16_t* out) {
    const uint8_t* p = proba[t][kBands[n]][ctx];
    for (; n < 16; ++n) {
      if (!b.get(p[0])) return n;
      while (!b.get(p[1])) {
        p = proba[t][kBands[++n]][0];
        if (n == 16) return 16;
      }
      int v;
      const uint8_t(*next)[11] = proba[t][kBands[n + 1]];
      if (!b.get(p[2])) { v = 1; p = next[1]; }
      else { v = large_value(b, p); p = next[2]; }
      out[kZigzag[n]] = (int16_t)((b.bit() ? -v : v) * dq[n > 0]);
    }
    return 16;
  }
};

}  // namespace detail

// the VP8 chunk's payload -> frame
inline bool parse(const uint8_t* d, size_t n, Frame& f) {
  using namespace detail;
  f = Frame();
  auto refuse = [&](const char* why) { f.error = why; f.mbs.clear(); f.coeffs.clear(); return false; };
  if (n < 10) return refuse(kNoKeyFrame);
  const uint32_t tag = d[0] | (d[1] << 8) | ((uint32_t)d[2] << 16);
  const size_t first = tag >> 5;
  if ((tag & 1) || ((tag >> 1) & 7) > 3 || !((tag >> 4) & 1)) return refuse(kNoKeyFrame);
  if (d[3] != 0x9d || d[4] != 0x01 || d[5] != 0x2a) return refuse(kNoKeyFrame);
  f.width = (d[6] | (d[7] << 8)) & 0x3fff;   // (the two bits on top: the horizontal scale, ignored)
  f.height = (d[8] | (d[9] << 8)) & 0x3fff;
  if (!f.width || !f.height || first >= n) return refuse(kNoKeyFrame);
  if (first > n - 10) return refuse(nullptr);
  Parser P;
  P.br = Bool(d + 10, first);
  P.br.bit();  // colour space
  P.br.bit();  // clamping type
  if (!P.segment_header() || !P.filter_header()) return refuse(nullptr);
  f.filter_type = P.level == 0 ? 0 : P.simple ? 1 : 2;
  {
    const uint8_t* buf = d + 10 + first;
    size_t left = n - 10 - first;
    P.nparts = 1 << P.br.literal(2);
    const size_t last = (size_t)P.nparts - 1;
    if (left < 3 * last) return refuse(nullptr);
    const uint8_t* sz = buf;
    const uint8_t* start = buf + 3 * last;
    left -= 3 * last;
    for (size_t p = 0; p < last; ++p, sz += 3) {
      size_t psize = sz[0] | (sz[1] << 8) | ((size_t)sz[2] << 16);
      if (psize > left) psize = left;
      P.part[p] = Bool(start, psize);
      start += psize;
      left -= psize;
    }
    P.part[last] = Bool(start, left);
    if (left == 0) return refuse(nullptr);
  }
  P.quant();
  P.br.bit();  // (key frames: the probabilities are not kept anyway)
  P.probas();
  P.strengths(f.filter_type);
  f.partitions = P.nparts;
  f.segments = P.update_map ? 4 : 1;

  const int mw = mb_w(f), mh = mb_h(f);
  struct Ctx { uint8_t nz = 0, nz_dc = 0; };
  std::vector<Ctx> top((size_t)mw);
  std::vector<uint8_t> intra_t((size_t)mw * 4, B_DC);
  f.mbs.assign((size_t)mw * mh, Mb());
  f.coeffs.reserve((size_t)mw * mh * 64);
  for (int y = 0; y < mh; ++y) {
    Mb* row = f.mbs.data() + (size_t)y * mw;
    uint8_t intra_l[4] = {B_DC, B_DC, B_DC, B_DC};
    for (int x = 0; x < mw; ++x) {  // a row of modes
      Mb& m = row[x];
      uint8_t* t = intra_t.data() + 4 * x;
      m.segment = !P.update_map ? 0 : !P.br.get(P.segment_proba[0]) ? (uint8_t)P.br.get(P.segment_proba[1]) : (uint8_t)(P.br.get(P.segment_proba[2]) + 2);
      m.skip = P.use_skip ? (uint8_t)P.br.get(P.skip_p) : 0;
      m.is_i4x4 = !P.br.get(145);
      if (!m.is_i4x4) {
        const int ymode = P.br.get(156) ? (P.br.get(128) ? TM_PRED : H_PRED) : (P.br.get(163) ? V_PRED : DC_PRED);
        m.modes[0] = (uint8_t)ymode;
        memset(t, ymode, 4);
        memset(intra_l, ymode, 4);
      } else {
        for (int by = 0; by < 4; ++by) {
          int ymode = intra_l[by];
          for (int bx = 0; bx < 4; ++bx) {
            const uint8_t* prob = kBModesProba + ((size_t)t[bx] * 10 + ymode) * 9;
            int i = kBModeTree[P.br.get(prob[0])];
            while (i > 0) i = kBModeTree[2 * i + P.br.get(prob[i])];
            ymode = -i;
            t[bx] = (uint8_t)ymode;
          }
          memcpy(m.modes + 4 * by, t, 4);
          intra_l[by] = (uint8_t)ymode;
        }
      }
      m.uvmode = !P.br.get(142) ? DC_PRED : !P.br.get(114) ? V_PRED : P.br.get(183) ? TM_PRED : H_PRED;
    }
    if (P.br.eof) return refuse(nullptr);
    Bool& tb = P.part[y & (P.nparts - 1)];
    Ctx left;
    for (int x = 0; x < mw; ++x) {  // and of tokens
      Mb& m = row[x];
      Ctx& mb = top[(size_t)x];
      int skip = m.skip;
      int16_t c[25 * 16];
      memset(c, 0, sizeof c);
      if (!skip) {
        const int s = m.segment;
        int firstc, type;
        int16_t dcs[16] = {};  // the WHT's outputs, to know which DCs are not zero
        if (!m.is_i4x4) {
          const int nz = P.block(tb, 1, mb.nz_dc + left.nz_dc, P.y2[s], 0, c + 24 * 16);
          mb.nz_dc = left.nz_dc = nz > 0;
          wht(c + 24 * 16, dcs, 1);
          firstc = 1; type = 0;
        } else {
          firstc = 0; type = 3;
        }
        uint32_t nz_y = 0, nz_uv = 0, any = 0;
        uint8_t tnz = mb.nz & 0x0f, lnz = left.nz & 0x0f;
        int16_t* dst = c;
        for (int by = 0; by < 4; ++by) {
          int l = lnz & 1;
          uint32_t codes = 0;
          for (int bx = 0; bx < 4; ++bx, dst += 16) {
            const int nz = P.block(tb, type, l + (tnz & 1), P.y1[s], firstc, dst);
            l = nz > firstc;
            tnz = (uint8_t)((tnz >> 1) | (l << 7));
            codes = (codes << 2) | (nz > 3 ? 3u : nz > 1 ? 2u : 0u);
            any |= nz > 1 || (m.is_i4x4 ? dst[0] : dcs[(dst - c) / 16]) != 0;
          }
          tnz >>= 4;
          lnz = (uint8_t)((lnz >> 1) | (l << 7));
          nz_y = (nz_y << 8) | codes;
        }
        uint32_t out_t = tnz, out_l = lnz >> 4;
        for (int ch = 0; ch < 4; ch += 2) {
          uint32_t codes = 0;
          tnz = (uint8_t)(mb.nz >> (4 + ch));
          lnz = (uint8_t)(left.nz >> (4 + ch));
          for (int by = 0; by < 2; ++by) {
            int l = lnz & 1;
            for (int bx = 0; bx < 2; ++bx, dst += 16) {
              const int nz = P.block(tb, 2, l + (tnz & 1), P.uv[s], 0, dst);
              l = nz > 0;
              tnz = (uint8_t)((tnz >> 1) | (l << 3));
              codes = (codes << 2) | (nz > 3 ? 3u : nz > 1 ? 2u : 0u);
              any |= nz > 1 || dst[0] != 0;
            }
            tnz >>= 2;
            lnz = (uint8_t)((lnz >> 1) | (l << 5));
          }
          nz_uv |= codes << (4 * ch);
          out_t |= (uint32_t)(tnz << 4) << ch;
          out_l |= (uint32_t)(lnz & 0xf0) << ch;
        }
        mb.nz = (uint8_t)out_t;
        left.nz = (uint8_t)out_l;
        m.nz_y = nz_y;
        m.nz_uv = nz_uv;
        skip = !any;
      } else {
        left.nz = mb.nz = 0;
        if (!m.is_i4x4) left.nz_dc = mb.nz_dc = 0;
      }
      if (f.filter_type) {
        const Parser::Strength& st = P.strength[m.segment][m.is_i4x4];
        m.level = st.level; m.ilevel = st.ilevel; m.hev = st.hev;
        m.inner = (uint8_t)(st.inner | !skip);
      }
      if (tb.eof) return refuse(nullptr);
      m.coeff_off = (uint32_t)(f.coeffs.size() / 16);
      for (int b = 0; b < 25; ++b) {
        const int16_t* blk = c + 16 * b;
        bool nonzero = false;
        for (int k = 0; k < 16; ++k) nonzero |= blk[k] != 0;
        if (!nonzero) continue;
        m.present |= 1u << b;
        f.coeffs.insert(f.coeffs.end(), blk, blk + 16);
      }
    }
  }
  return true;
}

// a whole file -> frame: the container through webp::parse, the VP8 payload through parse().  A frame whose size is not the
// VP8X canvas's is refused as libwebp refuses it, with a bare decode failure (the key-frame header itself is sound)
inline bool parse_file(const uint8_t* d, size_t n, Frame& f) {
  webp::Frame w;
  f = Frame();
  if (webp::parse(d, n, w)) { f.error = "webp: the file is lossless"; return false; }
  if (!w.vp8) { f.error = w.error; return false; }
  if (!parse(w.vp8, w.vp8_size, f)) return false;
  if (w.canvas_width && (w.canvas_width != f.width || w.canvas_height != f.height)) {
    f = Frame();
    return false;
  }
  return true;
}

// ----------------------------------------------------------------------------------------------------------- the pixel half
namespace detail {

constexpr int kBps = 32;  // the stride of a macroblock's work area

VP8_FN int mul1(int a) { return ((a * 20091) >> 16) + a; }
VP8_FN int mul2(int a) { return (a * 35468) >> 16; }
VP8_FN void add_px(uint8_t* p, int v) { *p = clip8(*p + v); }
// the full inverse DCT in 16-bit lanes (libwebp's SSE2 form): every sum wraps to int16_t
VP8_FN void transform_full(const int16_t* in, uint8_t* dst, int stride) {
  int16_t tmp[16];
  for (int i = 0; i < 4; ++i) {
    const int a = in[i] + in[8 + i], b = in[i] - in[8 + i];
    const int c = mul2(in[4 + i]) - mul1(in[12 + i]), d = mul1(in[4 + i]) + mul2(in[12 + i]);
    tmp[4 * i + 0] = (int16_t)(a + d); tmp[4 * i + 1] = (int16_t)(b + c); tmp[4 * i + 2] = (int16_t)(b - c); tmp[4 * i + 3] = (int16_t)(a - d);
  }
  for (int i = 0; i < 4; ++i) {
    const int dc = tmp[i] + 4;
    const int a = dc + tmp[8 + i], b = dc - tmp[8 + i];
    const int c = mul2(tmp[4 + i]) - mul1(tmp[12 + i]), d = mul1(tmp[4 + i]) + mul2(tmp[12 + i]);
    uint8_t* row = dst + i * stride;
    add_px(row + 0, (int16_t)(a + d) >> 3); add_px(row + 1, (int16_t)(b + c) >> 3);
    add_px(row + 2, (int16_t)(b - c) >> 3); add_px(row + 3, (int16_t)(a - d) >> 3);
  }
}
VP8_FN void transform_ac3(const int16_t* in, uint8_t* dst, int stride) {
  const int a = in[0] + 4, c4 = mul2(in[4]), d4 = mul1(in[4]), c1 = mul2(in[1]), d1 = mul1(in[1]);
  const int dcs[4] = {a + d4, a + c4, a - c4, a - d4};
  for (int y = 0; y < 4; ++y) {
    uint8_t* row = dst + y * stride;
    add_px(row + 0, (dcs[y] + d1) >> 3); add_px(row + 1, (dcs[y] + c1) >> 3);
    add_px(row + 2, (dcs[y] - c1) >> 3); add_px(row + 3, (dcs[y] - d1) >> 3);
  }
}
VP8_FN void transform_dc(const int16_t* in, uint8_t* dst, int stride) {
  const int dc = (in[0] + 4) >> 3;
  for (int y = 0; y < 4; ++y)
    for (int x = 0; x < 4; ++x) add_px(dst + y * stride + x, dc);
}
VP8_FN void transform_class(int code, const int16_t* in, uint8_t* dst, int stride) {
  if (code == 3) transform_full(in, dst, stride);
  else if (code == 2) transform_ac3(in, dst, stride);
  else if (in[0]) transform_dc(in, dst, stride);
}

VP8_FN int avg2(int a, int b) { return (a + b + 1) >> 1; }
VP8_FN int avg3(int a, int b, int c) { return (a + 2 * b + c + 2) >> 2; }
// one 4x4 sub-block at d (stride kBps); its neighbours stand around it
VP8_FN void predict4(int mode, uint8_t* d) {
  const uint8_t* top = d - kBps;
  const int X = top[-1], A = top[0], B = top[1], C = top[2], D = top[3], E = top[4], F = top[5], G = top[6], H = top[7];
  const int I = d[-1], J = d[-1 + kBps], K = d[-1 + 2 * kBps], L = d[-1 + 3 * kBps];
#define DST(x, y) d[(x) + (y) * kBps]
  switch (mode) {
    case B_DC: {
      const int dc = (A + B + C + D + I + J + K + L + 4) >> 3;
      for (int y = 0; y < 4; ++y) memset(d + y * kBps, dc, 4);
      break;
    }
    case B_TM: {
      const int left[4] = {I, J, K, L};
      for (int y = 0; y < 4; ++y)
        for (int x = 0; x < 4; ++x) DST(x, y) = clip8(top[x] + left[y] - X);
      break;
    }
    case B_VE: {
      const uint8_t v[4] = {(uint8_t)avg3(X, A, B), (uint8_t)avg3(A, B, C), (uint8_t)avg3(B, C, D), (uint8_t)avg3(C, D, E)};
      for (int y = 0; y < 4; ++y) memcpy(d + y * kBps, v, 4);
      break;
    }
    case B_HE:
      memset(d, avg3(X, I, J), 4); memset(d + kBps, avg3(I, J, K), 4); memset(d + 2 * kBps, avg3(J, K, L), 4); memset(d + 3 * kBps, avg3(K, L, L), 4);
      break;
    case B_RD:
      DST(0, 3) = (uint8_t)avg3(J, K, L);
      DST(1, 3) = DST(0, 2) = (uint8_t)avg3(I, J, K);
      DST(2, 3) = DST(1, 2) = DST(0, 1) = (uint8_t)avg3(X, I, J);
      DST(3, 3) = DST(2, 2) = DST(1, 1) = DST(0, 0) = (uint8_t)avg3(A, X, I);
      DST(3, 2) = DST(2, 1) = DST(1, 0) = (uint8_t)avg3(B, A, X);
      DST(3, 1) = DST(2, 0) = (uint8_t)avg3(C, B, A);
      DST(3, 0) = (uint8_t)avg3(D, C, B);
      break;
    case B_VR:
      DST(0, 0) = DST(1, 2) = (uint8_t)avg2(X, A);
      DST(1, 0) = DST(2, 2) = (uint8_t)avg2(A, B);
      DST(2, 0) = DST(3, 2) = (uint8_t)avg2(B, C);
      DST(3, 0) = (uint8_t)avg2(C, D);
      DST(0, 3) = (uint8_t)avg3(K, J, I);
      DST(0, 2) = (uint8_t)avg3(J, I, X);
      DST(0, 1) = DST(1, 3) = (uint8_t)avg3(I, X, A);
      DST(1, 1) = DST(2, 3) = (uint8_t)avg3(X, A, B);
      DST(2, 1) = DST(3, 3) = (uint8_t)avg3(A, B, C);
      DST(3, 1) = (uint8_t)avg3(B, C, D);
      break;
    case B_LD:
      DST(0, 0) = (uint8_t)avg3(A, B, C);
      DST(1, 0) = DST(0, 1) = (uint8_t)avg3(B, C, D);
      DST(2, 0) = DST(1, 1) = DST(0, 2) = (uint8_t)avg3(C, D, E);
      DST(3, 0) = DST(2, 1) = DST(1, 2) = DST(0, 3) = (uint8_t)avg3(D, E, F);
      DST(3, 1) = DST(2, 2) = DST(1, 3) = (uint8_t)avg3(E, F, G);
      DST(3, 2) = DST(2, 3) = (uint8_t)avg3(F, G, H);
      DST(3, 3) = (uint8_t)avg3(G, H, H);
      break;
    case B_VL:
      DST(0, 0) = (uint8_t)avg2(A, B);
      DST(1, 0) = DST(0, 2) = (uint8_t)avg2(B, C);
      DST(2, 0) = DST(1, 2) = (uint8_t)avg2(C, D);
      DST(3, 0) = DST(2, 2) = (uint8_t)avg2(D, E);
      DST(0, 1) = (uint8_t)avg3(A, B, C);
      DST(1, 1) = DST(0, 3) = (uint8_t)avg3(B, C, D);
      DST(2, 1) = DST(1, 3) = (uint8_t)avg3(C, D, E);
      DST(3, 1) = DST(2, 3) = (uint8_t)avg3(D, E, F);
      DST(3, 2) = (uint8_t)avg3(E, F, G);
      DST(3, 3) = (uint8_t)avg3(F, G, H);
      break;
    case B_HD:
      DST(0, 0) = DST(2, 1) = (uint8_t)avg2(I, X);
      DST(0, 1) = DST(2, 2) = (uint8_t)avg2(J, I);
      DST(0, 2) = DST(2, 3) = (uint8_t)avg2(K, J);
      DST(0, 3) = (uint8_t)avg2(L, K);
      DST(3, 0) = (uint8_t)avg3(A, B, C);
      DST(2, 0) = (uint8_t)avg3(X, A, B);
      DST(1, 0) = DST(3, 1) = (uint8_t)avg3(I, X, A);
      DST(1, 1) = DST(3, 2) = (uint8_t)avg3(J, I, X);
      DST(1, 2) = DST(3, 3) = (uint8_t)avg3(K, J, I);
      DST(1, 3) = (uint8_t)avg3(L, K, J);
      break;
    default:  // B_HU
      DST(0, 0) = (uint8_t)avg2(I, J);
      DST(2, 0) = DST(0, 1) = (uint8_t)avg2(J, K);
      DST(2, 1) = DST(0, 2) = (uint8_t)avg2(K, L);
      DST(1, 0) = (uint8_t)avg3(I, J, K);
      DST(3, 0) = DST(1, 1) = (uint8_t)avg3(J, K, L);
      DST(3, 1) = DST(1, 2) = (uint8_t)avg3(K, L, L);
      DST(3, 2) = DST(2, 2) = DST(0, 3) = DST(1, 3) = DST(2, 3) = DST(3, 3) = (uint8_t)L;
      break;
  }
#undef DST
}
// a size x size block (16 luma, 8 chroma) at d, stride kBps; has_top / has_left: the macroblock is not on that frame border
inline void predict_square(int mode, uint8_t* d, int size, bool has_top, bool has_left) {
  const uint8_t* top = d - kBps;
  if (mode == DC_PRED) {
    int dc = 0x80;
    const int shift = size == 16 ? 3 : 2;  // log2(size) - 1
    if (has_top || has_left) {
      int sum = 0;
      if (has_top) for (int k = 0; k < size; ++k) sum += top[k];
      if (has_left) for (int k = 0; k < size; ++k) sum += d[-1 + k * kBps];
      dc = has_top && has_left ? (sum + size) >> (shift + 2) : (sum + (size >> 1)) >> (shift + 1);
    }
    for (int y = 0; y < size; ++y) memset(d + y * kBps, dc, (size_t)size);
  } else if (mode == TM_PRED) {
    const int X = top[-1];
    for (int y = 0; y < size; ++y)
      for (int x = 0; x < size; ++x) d[x + y * kBps] = clip8(top[x] + d[-1 + y * kBps] - X);
  } else if (mode == V_PRED) {
    for (int y = 0; y < size; ++y) memcpy(d + y * kBps, top, (size_t)size);
  } else {
    for (int y = 0; y < size; ++y) memset(d + y * kBps, d[-1 + y * kBps], (size_t)size);
  }
}

// the neighbours of macroblock (x, y) of a plane (block: 16 or 8 pixels) into the work area around d
inline void fetch_neighbours(const uint8_t* plane, int stride, int x, int y, int block, int mbw, uint8_t* d, bool top_right) {
  const uint8_t* at = plane + (size_t)y * block * stride + (size_t)x * block;
  if (y > 0) {
    memcpy(d - kBps, at - stride, (size_t)block);
    d[-kBps - 1] = x > 0 ? at[-stride - 1] : 129;
    if (top_right) {
      if (x < mbw - 1) memcpy(d - kBps + 16, at - stride + 16, 4);
      else memset(d - kBps + 16, at[-stride + 15], 4);
    }
  } else {
    memset(d - kBps - 1, 127, (size_t)block + 1 + (top_right ? 4 : 0));
  }
  for (int k = 0; k < block; ++k) d[-1 + k * kBps] = x > 0 ? at[(size_t)k * stride - 1] : 129;
}
inline void store_block(uint8_t* plane, int stride, int x, int y, int block, const uint8_t* d) {
  uint8_t* at = plane + (size_t)y * block * stride + (size_t)x * block;
  for (int k = 0; k < block; ++k) memcpy(at + (size_t)k * stride, d + k * kBps, (size_t)block);
}

// ---- the loop filter on a plane; p: the first pixel behind the edge, step: across the edge
VP8_FN int sclip1(int v) { return v < -128 ? -128 : v > 127 ? 127 : v; }
VP8_FN int sclip2(int v) { return v < -16 ? -16 : v > 15 ? 15 : v; }
VP8_FN void filter2(uint8_t* p, int step) {
  const int p1 = p[-2 * step], p0 = p[-step], q0 = p[0], q1 = p[step];
  const int a = 3 * (q0 - p0) + sclip1(p1 - q1);
  const int a1 = sclip2((a + 4) >> 3), a2 = sclip2((a + 3) >> 3);
  p[-step] = clip8(p0 + a2);
  p[0] = clip8(q0 - a1);
}
VP8_FN void filter4(uint8_t* p, int step) {
  const int p1 = p[-2 * step], p0 = p[-step], q0 = p[0], q1 = p[step];
  const int a = 3 * (q0 - p0);
  const int a1 = sclip2((a + 4) >> 3), a2 = sclip2((a + 3) >> 3), a3 = (a1 + 1) >> 1;
  p[-2 * step] = clip8(p1 + a3);
  p[-step] = clip8(p0 + a2);
  p[0] = clip8(q0 - a1);
  p[step] = clip8(q1 - a3);
}
VP8_FN void filter6(uint8_t* p, int step) {
  const int p2 = p[-3 * step], p1 = p[-2 * step], p0 = p[-step], q0 = p[0], q1 = p[step], q2 = p[2 * step];
  const int a = sclip1(3 * (q0 - p0) + sclip1(p1 - q1));
  const int a1 = (27 * a + 63) >> 7, a2 = (18 * a + 63) >> 7, a3 = (9 * a + 63) >> 7;
  p[-3 * step] = clip8(p2 + a3);
  p[-2 * step] = clip8(p1 + a2);
  p[-step] = clip8(p0 + a1);
  p[0] = clip8(q0 - a1);
  p[step] = clip8(q1 - a2);
  p[2 * step] = clip8(q2 - a3);
}
VP8_FN bool hev(const uint8_t* p, int step, int t) { return abs(p[-2 * step] - p[-step]) > t || abs(p[step] - p[0]) > t; }
VP8_FN bool needs_filter(const uint8_t* p, int step, int t) { return 4 * abs(p[-step] - p[0]) + abs(p[-2 * step] - p[step]) <= t; }
VP8_FN bool needs_filter2(const uint8_t* p, int step, int t, int it) {
  if (!needs_filter(p, step, t)) return false;
  return abs(p[-4 * step] - p[-3 * step]) <= it && abs(p[-3 * step] - p[-2 * step]) <= it && abs(p[-2 * step] - p[-step]) <= it &&
         abs(p[3 * step] - p[2 * step]) <= it && abs(p[2 * step] - p[step]) <= it && abs(p[step] - p[0]) <= it;
}
// one position of an edge: simple; normal on a macroblock edge (mb_edge) or an inner one
VP8_FN void filter_simple(uint8_t* p, int step, int thresh) {
  if (needs_filter(p, step, 2 * thresh + 1)) filter2(p, step);
}
VP8_FN void filter_normal(uint8_t* p, int step, int thresh, int ithresh, int hev_t, bool mb_edge) {
  if (!needs_filter2(p, step, 2 * thresh + 1, ithresh)) return;
  if (hev(p, step, hev_t)) filter2(p, step);
  else if (mb_edge) filter6(p, step);
  else filter4(p, step);
}
// one position of all edges of a macroblock that run in one direction: p is that position on the macroblock edge, `across`
// leads over the edges.  outer: the macroblock edge is filtered too (it is not the frame's); chroma: p lies in U or V, which
// the simple filter leaves alone and which have one inner edge.  Positions of an edge do not depend on one another.
VP8_FN void filter_line(const Mb& m, int filter_type, bool outer, uint8_t* p, int across, bool chroma) {
  if (chroma && filter_type != 2) return;
  const int limit = 2 * m.level + m.ilevel;
  for (int e = outer ? 0 : 1; e < (m.inner ? (chroma ? 2 : 4) : 1); ++e) {
    const int thresh = e == 0 ? limit + 4 : limit;
    if (filter_type == 1) filter_simple(p + 4 * e * across, across, thresh);
    else filter_normal(p + 4 * e * across, across, thresh, m.ilevel, m.hev, e == 0);
  }
}

// ---- fancy upsampling and libwebp's YUV -> BGR
VP8_FN int mult_hi(int v, int coeff) { return (v * coeff) >> 8; }
VP8_FN uint8_t clip_fix(int v) { return (v & ~16383) == 0 ? (uint8_t)(v >> 6) : v < 0 ? 0 : 255; }
VP8_FN void yuv_to_bgr(int y, int u, int v, uint8_t* bgr) {
  bgr[0] = clip_fix(mult_hi(y, 19077) + mult_hi(u, 33050) - 17685);
  bgr[1] = clip_fix(mult_hi(y, 19077) - mult_hi(u, 6419) - mult_hi(v, 13320) + 8708);
  bgr[2] = clip_fix(mult_hi(y, 19077) + mult_hi(v, 26149) - 14234);
}
// the chroma sample of pixel (x, y): the nearest sample N, its neighbour H in the row, V in the column, D across
VP8_FN int upsample(const uint8_t* c, int stride, int x, int y, int width, int cw, int ch) {
  const int cx = x >> 1, cy = y >> 1;
  int fy = (y & 1) ? cy + 1 : cy - 1;
  fy = fy < 0 ? 0 : fy > ch - 1 ? ch - 1 : fy;
  const int N = c[(size_t)cy * stride + cx], V = c[(size_t)fy * stride + cx];
  if (x == 0 || (x == width - 1 && !(width & 1))) return (3 * N + V + 2) >> 2;
  const int fx = (x & 1) ? cx + 1 : cx - 1;  // (in range: the two columns without a neighbour went above)
  (void)cw;
  const int H = c[(size_t)cy * stride + fx], D = c[(size_t)fy * stride + fx];
  return (((N + 3 * H + 3 * V + D + 8) >> 3) + N) >> 1;
}

}  // namespace detail

// the three planes of a sound frame, reconstructed and filtered: macroblock-aligned, strides 16 * mb_w and 8 * mb_w
inline void planes(const Frame& f, std::vector<uint8_t>& Y, std::vector<uint8_t>& U, std::vector<uint8_t>& V) {
  using namespace detail;
  const int mw = mb_w(f), mh = mb_h(f), ys = 16 * mw, cs = 8 * mw;
  Y.assign((size_t)ys * 16 * mh, 0);
  U.assign((size_t)cs * 8 * mh, 0);
  V.assign((size_t)cs * 8 * mh, 0);
  uint8_t ybuf[kBps * 17 + 8], ubuf[kBps * 9 + 8], vbuf[kBps * 9 + 8];
  uint8_t *yd = ybuf + kBps + 4, *ud = ubuf + kBps + 4, *vd = vbuf + kBps + 4;
  for (int y = 0; y < mh; ++y)
    for (int x = 0; x < mw; ++x) {
      const Mb& m = f.mbs[(size_t)y * mw + x];
      int16_t c[25 * 16];
      memset(c, 0, sizeof c);
      const int16_t* src = f.coeffs.data() + (size_t)m.coeff_off * 16;
      for (int b = 0; b < 25; ++b)
        if (m.present >> b & 1) { memcpy(c + 16 * b, src, 32); src += 16; }
      if (!m.is_i4x4) wht(c + 24 * 16, c);
      fetch_neighbours(Y.data(), ys, x, y, 16, mw, yd, true);
      fetch_neighbours(U.data(), cs, x, y, 8, mw, ud, false);
      fetch_neighbours(V.data(), cs, x, y, 8, mw, vd, false);
      if (m.is_i4x4) {
        for (int r = 1; r < 4; ++r) memcpy(yd + (4 * r - 1) * kBps + 16, yd - kBps + 16, 4);
      } else {
        predict_square(m.modes[0], yd, 16, y > 0, x > 0);
      }
      for (int n = 0; n < 16; ++n) {
        uint8_t* d = yd + (n >> 2) * 4 * kBps + (n & 3) * 4;
        if (m.is_i4x4) predict4(m.modes[n], d);
        transform_class((int)(m.nz_y >> (30 - 2 * n)) & 3, c + 16 * n, d, kBps);
      }
      predict_square(m.uvmode, ud, 8, y > 0, x > 0);
      predict_square(m.uvmode, vd, 8, y > 0, x > 0);
      for (int p = 0; p < 2; ++p) {
        const uint32_t codes = (m.nz_uv >> (8 * p)) & 0xff;
        uint8_t* d = p ? vd : ud;
        const int16_t* in = c + 16 * (16 + 4 * p);
        for (int n = 0; n < 4; ++n) {
          uint8_t* at = d + (n >> 1) * 4 * kBps + (n & 1) * 4;
          if (codes & 0xaa) transform_full(in + 16 * n, at, kBps);
          else if (in[16 * n]) transform_dc(in + 16 * n, at, kBps);
        }
      }
      store_block(Y.data(), ys, x, y, 16, yd);
      store_block(U.data(), cs, x, y, 8, ud);
      store_block(V.data(), cs, x, y, 8, vd);
    }
  if (!f.filter_type) return;
  for (int y = 0; y < mh; ++y)
    for (int x = 0; x < mw; ++x) {
      const Mb& m = f.mbs[(size_t)y * mw + x];
      if (!m.level) continue;
      uint8_t* yp = Y.data() + (size_t)y * 16 * ys + x * 16;
      uint8_t* up = U.data() + (size_t)y * 8 * cs + x * 8;
      uint8_t* vp = V.data() + (size_t)y * 8 * cs + x * 8;
      for (int k = 0; k < 16; ++k) filter_line(m, f.filter_type, x > 0, yp + (size_t)k * ys, 1, false);  // vertical edges, row k
      for (int k = 0; k < 8; ++k) {
        filter_line(m, f.filter_type, x > 0, up + (size_t)k * cs, 1, true);
        filter_line(m, f.filter_type, x > 0, vp + (size_t)k * cs, 1, true);
      }
      for (int k = 0; k < 16; ++k) filter_line(m, f.filter_type, y > 0, yp + k, ys, false);  // horizontal edges, column k
      for (int k = 0; k < 8; ++k) {
        filter_line(m, f.filter_type, y > 0, up + k, cs, true);
        filter_line(m, f.filter_type, y > 0, vp + k, cs, true);
      }
    }
}

// the exact-parity host stage: frame -> packed BGR, height x width; false when fault(frame)
inline bool pixels(const Frame& f, std::vector<uint8_t>& bgr) {
  if (fault(f)) return false;
  std::vector<uint8_t> Y, U, V;
  planes(f, Y, U, V);
  const int w = f.width, h = f.height, ys = 16 * mb_w(f), cs = 8 * mb_w(f), cw = (w + 1) >> 1, ch = (h + 1) >> 1;
  bgr.resize((size_t)w * h * 3);
  for (int y = 0; y < h; ++y)
    for (int x = 0; x < w; ++x)
      detail::yuv_to_bgr(Y[(size_t)y * ys + x], detail::upsample(U.data(), cs, x, y, w, cw, ch), detail::upsample(V.data(), cs, x, y, w, cw, ch),
                         bgr.data() + ((size_t)y * w + x) * 3);
  return true;
}

}  // namespace vp8
}  // namespace PaddleOCR
