// Host-visible launch interface of kernels_jpeg.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ocr {

struct JpegPlaneDesc {       // one component of one image
  const int16_t* coef;       // device: bw*bh blocks x 64 quantised coefficients, natural order
  uint16_t quant[64];        // its quantisation table, natural order
  uint8_t* plane;            // device: (bh*8) x (bw*8) samples out
  int bw, bh;
  long first_block;          // prefix sum of blocks over the launch's planes
};
struct JpegImageDesc {
  const uint8_t* plane[3];
  int stride[3], dw[3], dh[3];
  uint8_t* bgr;              // device: packed BGR out, rows x cols - cols x rows when orient >= 5
  int rows, cols, ncomp, hmax, vmax;  // rows / cols: the stored size
  int orient;                // EXIF orientation 1..8 (the table in host/jpeg_decode.h)
};
// An image of the general kinds: 1, 3 or 4 components, each with its own upsampling, and a colour space.
enum JpegUpsample { kJpegCopy = 0, kJpegFancyH2V1 = 1, kJpegFancyH2V2 = 2, kJpegFancyH1V2 = 3, kJpegBox = 4 };  // host/jpeg_decode.h Upsample
enum JpegColor { kJpegGrey = 0, kJpegYCbCr = 1, kJpegRGB = 2, kJpegCMYK = 3, kJpegYCCK = 4 };                   // ocr_jpeg_color
struct JpegGenDesc {
  const uint8_t* plane[4];
  int stride[4], dw[4], dh[4];
  uint8_t method[4];         // JpegUpsample, chosen on the host from (hexp, vexp) and dw as jdsample.c chooses it
  uint8_t hexp[4], vexp[4];  // hmax / h, vmax / v: 1..4
  uint8_t* bgr;              // device: packed BGR out, rows x cols - cols x rows when orient >= 5
  int rows, cols, ncomp;     // rows / cols: the stored size
  int color;                 // JpegColor
  int orient;
};
// The pixel stage has one kernel per kind of image, so that an image runs the code it ran before there was an
// orientation or another sampling.  Grey and YCbCr 4:4:4 / 4:2:2 / 4:2:0 (JpegImageDesc): 0 = as stored (1), 1 = rows stay
// rows (2..4), 2 = rows become columns (5..8).  Everything else (JpegGenDesc): 3 = rows stay rows (1..4), 4 = rows become
// columns (5..8).
constexpr int kJpegKinds = 5;
constexpr int kJpegGenKind = 3;  // the first kind whose descriptors are JpegGenDesc
inline int jpeg_output_kind(int orient) { return orient >= 5 ? 2 : orient >= 2 ? 1 : 0; }
inline int jpeg_general_kind(int orient) { return orient >= 5 ? 4 : 3; }
constexpr int kJpegTile = 64;  // side of the square of stored pixels one workgroup transposes
// workgroups that one image needs in the kernel of its kind
inline long jpeg_output_blocks(int rows, int cols, int orient) {
  if (orient >= 5) return (long)((rows + kJpegTile - 1) / kJpegTile) * ((cols + kJpegTile - 1) / kJpegTile);
  return ((long)rows * cols + 255) / 256;
}
inline long jpeg_output_blocks(const JpegImageDesc& d) { return jpeg_output_blocks(d.rows, d.cols, d.orient); }
// The two stages of one batch.  The image descriptors are ordered by kind: kind k < kJpegGenKind is imgs[first[k]] ..
// + count[k], kind k >= kJpegGenKind is gens[first[k]] .. + count[k], and blocks[k] the largest jpeg_output_blocks among
// them; a kind without images is not launched.
struct JpegLaunch {
  int ndesc = 0;
  long idct_blocks = 0;
  int first[kJpegKinds] = {}, count[kJpegKinds] = {};
  long blocks[kJpegKinds] = {};
};
void launch_jpeg_idct(const JpegPlaneDesc* descs, int ndesc, long total_blocks, hipStream_t s);
void launch_jpeg_output(const JpegImageDesc* imgs, const JpegGenDesc* gens, const JpegLaunch& L, hipStream_t s);

}  // namespace ocr
