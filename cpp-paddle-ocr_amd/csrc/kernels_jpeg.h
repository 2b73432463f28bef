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
// The pixel stage has one kernel per kind of orientation, so that an image stored upright runs the code it ran before
// there was an orientation: 0 = as stored (1), 1 = rows stay rows (2..4), 2 = rows become columns (5..8).
constexpr int kJpegKinds = 3;
inline int jpeg_output_kind(int orient) { return orient >= 5 ? 2 : orient >= 2 ? 1 : 0; }
constexpr int kJpegTile = 64;  // side of the square of stored pixels one workgroup transposes
// workgroups that one image needs in the kernel of its kind
inline long jpeg_output_blocks(const JpegImageDesc& d) {
  if (jpeg_output_kind(d.orient) == 2) return (long)((d.rows + kJpegTile - 1) / kJpegTile) * ((d.cols + kJpegTile - 1) / kJpegTile);
  return ((long)d.rows * d.cols + 255) / 256;
}
// The two stages of one batch.  The image descriptors are ordered by kind: kind k is imgs[first[k]] .. + count[k], and
// blocks[k] the largest jpeg_output_blocks among them; a kind without images is not launched.
struct JpegLaunch {
  int ndesc = 0;
  long idct_blocks = 0;
  int first[kJpegKinds] = {}, count[kJpegKinds] = {};
  long blocks[kJpegKinds] = {};
};
void launch_jpeg_idct(const JpegPlaneDesc* descs, int ndesc, long total_blocks, hipStream_t s);
void launch_jpeg_output(const JpegImageDesc* imgs, const JpegLaunch& L, hipStream_t s);

}  // namespace ocr
