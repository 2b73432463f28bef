// Host-visible launch interface of kernels_j2k.hip: the sample half of the JPEG 2000 decoder - dequantisation, the multi-level
// inverse wavelet transform (5/3 in int32, 9/7 in float32 without contraction), inverse component transform, level shift, clamp
// and BGR store - to the bytes of j2k::pixels (host/j2k_decode.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../host/j2k_decode.h"  // the geometry and the sample arithmetic, stated once for host and device

namespace ocr {

constexpr int kJ2kBlock = 256;   // threads of every workgroup
constexpr int kJ2kHalo = 4;      // samples either side of a window: the 9/7 has four lifting steps that reach one sample each
constexpr int kJ2kRowWin = 256;  // horizontal pass: window of a row in LDS, kJ2kRowWin - 2 * kJ2kHalo of them written
constexpr int kJ2kRows = 4;      // rows of a horizontal workgroup: a wave a row
constexpr int kJ2kCols = 64;     // vertical pass: columns of a strip - a wave reads 256 contiguous bytes of a row
constexpr int kJ2kColWin = 64;   // rows of a strip's window in LDS, kJ2kColWin - 2 * kJ2kHalo of them written

struct J2kTc {  // a tile-component of the batch
  int x0, y0, x1, y1, levels, transform;
  uint32_t plane;     // where its (x1 - x0) * (y1 - y0) samples start in each of the three planes
  uint32_t step_off;  // into the batch's steps
};
struct J2kTile {  // the components of a tile are finished together
  uint32_t tc[3];
  int ncomp, mct, prec, transform, chan[3];
  int img_w, ox, oy;  // the image's width, the tile's origin inside the image
  uint8_t* dst;       // device: packed BGR of the image, any alignment
};
struct J2kUnit { uint32_t job; int r, p, q; };  // a workgroup's share: job (tile-component or tile), resolution produced, window origin
struct J2kBatch {
  const int32_t* a;  // device: coefficients as uploaded (band arrangement), never written
  int32_t* b;        // device: rows done
  int32_t* r;        // device: the resolution reconstructed so far, top-left of each plane
  const float* steps;
  const J2kTc* tcs;
  const J2kTile* tiles;
  const J2kUnit* units;
};
struct J2kStep { uint32_t h_first, h_count, v_first, v_count; };  // ranges of units

// steps[0 .. nsteps): horizontal then vertical pass of one level for every image, tile and component that has it; then the
// finishing pass (the last level's columns, component transform, shift, clamp, BGR) over fin_count units from fin_first.
void launch_j2k(const J2kBatch& batch, const J2kStep* steps, int nsteps, uint32_t fin_first, uint32_t fin_count, hipStream_t s);

}  // namespace ocr
