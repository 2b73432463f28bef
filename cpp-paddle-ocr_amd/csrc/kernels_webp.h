// Host-visible launch interface of kernels_webp.hip: the pixel half of the lossless WebP decoder (the inverse transforms of
// VP8L - spatial predictor, cross-colour, add-green, palette with pixel bundling - to packed BGR as cv::imdecode(IMREAD_COLOR)
// gives it through libwebp).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ocr {

constexpr int kWebpKinds = 2;           // frames with a predictor (one wave an image), frames without (streaming): a launch each
constexpr int kWebpBand = 64;           // rows of a band = lanes of a wave
constexpr int kWebpTile = 64;           // coded pixels per row that one LDS flush writes
constexpr int kWebpRing = 3 * kWebpTile;  // coded pixels per ring row (kernels_webp.hip says why three tiles)
constexpr int kWebpBlock = 256;         // threads of a streaming workgroup
constexpr int kWebpGroup = 4;           // output pixels of a streaming lane: 12 bytes, three dwords
constexpr int kWebpMaxGrid = 1 << 11;   // workgroups of a streaming launch; the units beyond are walked with a grid stride

enum WebpOp { WEBP_OP_CROSS = 1, WEBP_OP_GREEN = 2 };

struct WebpImageDesc {
  const uint32_t* argb;    // device: the entropy-decoded image, coded_width x height
  const uint32_t* pred;    // device: the predictor's sub-image (mode in bits 8 .. 11), null without a predictor
  const uint32_t* cross;   // device: the cross-colour sub-image, null without
  uint32_t* recon;         // device: a row of coded_width dwords for every band that another band follows
  uint8_t* bgr;            // device: packed BGR out, height x width, any alignment
  unsigned long long first_unit;  // streaming: a unit is one span (kWebpBlock x kWebpGroup pixels) of one output row
  unsigned spans;                 // of a row
  int width, height, coded_width;
  int pred_bits, cross_bits;
  int index_bits;          // -1: no palette; else a coded pixel's green byte holds 2^index_bits indices
  // the pointwise transforms in the order they are applied: in front of the predictor (to the residual as it is loaded; all
  // of them when there is no predictor) and behind it (at flush time)
  int npre, pre[2], npost, post[2];
  uint32_t palette[256];   // B | G << 8 | R << 16, zero beyond the file's entries
};

// rows of `recon` a frame needs: one per band that is followed by another (bands take 64 rows, then 63 new ones each)
inline int webp_recon_rows(int height) { return height <= kWebpBand ? 0 : (height - kWebpBand + kWebpBand - 2) / (kWebpBand - 1); }

// kind 0: imgs[0 .. nimg) have a predictor, one workgroup (one wave) each.  kind 1: they have none, total_units spans in all.
void launch_webp(int kind, const WebpImageDesc* imgs, int nimg, unsigned long long total_units, hipStream_t s);

}  // namespace ocr
