// The pixel half of the PNG decoder on the device: unfiltering, conversion to packed BGR, Adam7 placement, in one pass
// over the inflated stream (the host keeps the container and zlib's inflate: host/png_decode.h).
//
// Unfiltering is a dependency chain - Recon(x) needs a = Recon(x - bpp), b = Prior(x), c = Prior(x - bpp) - and Average
// and Paeth are not associative, so there is no scan to run along a row.  What is parallel: the anti-diagonal of a block
// of rows, the segments of an image (maximal runs of rows that never look outside the run: a None or Sub row starts one)
// and the images of a batch.
//
//   - a workgroup is ONE wave and takes one segment; it walks the segment in bands of 64 rows, lane l owning row r0 + l
//   - at step t lane l reconstructs filter unit t - l of its row (a unit = the bpp bytes of a pixel; one byte, several
//     pixels, at depths below 8).  b comes from the lane above by a one-lane shift of the previous step's results, c is
//     the b of the step before, a the lane's own last result: registers only
//   - bands after a segment's first take 63 new rows: lane 0 REPLAYS the last row of the band before, which that band's
//     lane 63 wrote, reconstructed, to `recon` (the only intermediate bytes that reach memory), and feeds lane 1 as any
//     row above would.  A segment's first row has no row above: lane 0's b is zero
//   - the unit loads of 8 steps are issued together ahead of the 8 dependent steps
//   - at any step the 64 lanes sit in 64 different rows, so a store per lane would be 3 bytes to each of 64 lines.  The
//     bytes a pixel keeps (1 for grey / index, 3 for colour: low bytes of 16-bit samples and alpha are dropped here)
//     go to an LDS ring of 64 rows x 128 units instead; when every lane has passed a tile of 64 units - step 64j + 126
//     for tile j, while lane 0 is still inside tile j + 1 - the tile is written out row by row, lanes along the row:
//     contiguous bytes (strided by the pass's dx for Adam7).  Conversion happens there: bit replication, palette, grey
//     to three channels, RGB to BGR.  A ring row is 128 * kept + 4 + kept bytes: the skewed front (lane l at unit
//     t - l) then advances by 32 * kept + 1 dwords per lane, one bank per lane, and the row-wise reads of the flush are
//     consecutive bytes.
#include "kernels_png.h"

namespace ocr {
namespace {

__device__ __forceinline__ int png_paeth(int a, int b, int c) {
  const int p = a + b - c, pa = abs(p - a), pb = abs(p - b), pc = abs(p - c);
  return pa <= pb && pa <= pc ? a : pb <= pc ? b : c;
}

template <int BPP>
__global__ void __launch_bounds__(kPngBand) png_pixel_kernel(const PngImageDesc* __restrict__ imgs, const PngWork* __restrict__ work, int nwork) {
  constexpr int KB = BPP <= 2 ? 1 : 3;         // bytes of a unit that the output needs
  constexpr int RING = 2 * kPngTile;           // units per ring row
  constexpr int RS = RING * KB + 4 + KB;       // bytes per ring row
  constexpr int G = 8;                         // steps per group of loads (divides kPngTile)
  constexpr int NW = (BPP + 3) / 4;
  __shared__ uint8_t ring[kPngBand * RS];
  if ((int)blockIdx.x >= nwork) return;
  const PngWork w = work[blockIdx.x];
  const PngImageDesc& im = imgs[w.img];
  const PngPassDesc q = im.pass[w.pass];
  const int lane = threadIdx.x;
  const int U = q.rowbytes / BPP;              // units per row
  const size_t stride = (size_t)q.rowbytes + 1;
  const uint8_t* base = im.data + q.offset;
  uint8_t* rbase = im.recon + q.offset;
  const int seg_end = w.first_row + w.rows;
  const int depth = im.depth, ctype = im.ctype, width = im.width;
  const int ppu_log = depth == 1 ? 3 : depth == 2 ? 2 : depth == 4 ? 1 : 0, ppu = 1 << ppu_log;  // pixels per unit
  const int ntiles = (U + kPngTile - 1) / kPngTile;
  uint8_t* const out0 = im.bgr + ((size_t)q.y0 * width + q.x0) * 3;

  for (int first = w.first_row, band = 0; first < seg_end; ++band) {
    const int row0 = band == 0 ? first : first - 1;  // lane 0's row: the band's first, or the replayed one
    const int nl = min(kPngBand, seg_end - row0);
    const int next = row0 + nl;
    const bool more = next < seg_end;              // (then nl == kPngBand)
    const bool active = lane < nl, replay = band > 0 && lane == 0, saver = more && lane == nl - 1;
    const size_t row_off = active ? (size_t)(row0 + lane) * stride : 0;
    const uint8_t* src = (replay ? rbase : base) + row_off + 1;
    uint8_t* save = rbase + row_off + 1;
    const int ft = active && !replay ? base[row_off] : 0;  // a replayed row is already reconstructed: None

    // tile j of the ring -> the image, row by row (uniform: every lane calls it)
    auto flush = [&](int tile) {
      const int p_lo = (tile * kPngTile) << ppu_log, p_hi = min(min((tile + 1) * kPngTile, U) << ppu_log, q.cols);
      for (int r = band > 0 ? 1 : 0; r < nl; ++r) {
        uint8_t* orow = out0 + (size_t)(row0 + r) * q.dy * width * 3;
        const uint8_t* rr = ring + r * RS;
        for (int p = p_lo + lane; p < p_hi; p += kPngBand) {
          const int u = p >> ppu_log;
          const uint8_t* s = rr + (u & (RING - 1)) * KB;
          uint8_t B, Gr, R;
          if (KB == 1) {
            int v = s[0];
            if (depth < 8) v = (v >> ((ppu - 1 - (p & (ppu - 1))) * depth)) & ((1 << depth) - 1);
            if (ctype == 3) { R = im.palette[3 * v]; Gr = im.palette[3 * v + 1]; B = im.palette[3 * v + 2]; }
            else { if (depth < 8) v *= 255 / ((1 << depth) - 1); B = Gr = R = (uint8_t)v; }
          } else {
            R = s[0]; Gr = s[1]; B = s[2];
          }
          uint8_t* o = orow + (size_t)p * q.dx * 3;
          o[0] = B; o[1] = Gr; o[2] = R;
        }
      }
    };

    uint8_t res[BPP], bold[BPP];
#pragma unroll
    for (int i = 0; i < BPP; ++i) res[i] = bold[i] = 0;
    const int nsteps = U + nl - 1;
    int flushed = 0;
    for (int t0 = 0; t0 < nsteps; t0 += G) {
      uint8_t raw[G][BPP];
#pragma unroll
      for (int g = 0; g < G; ++g) {
        const int u = t0 + g - lane;
#pragma unroll
        for (int i = 0; i < BPP; ++i) raw[g][i] = 0;
        if (active && u >= 0 && u < U) {
#pragma unroll
          for (int i = 0; i < BPP; ++i) raw[g][i] = src[(size_t)u * BPP + i];
        }
      }
#pragma unroll
      for (int g = 0; g < G; ++g) {
        const int u = t0 + g - lane;
        const bool valid = active && u >= 0 && u < U;
        // b: what the lane above finished one step ago
        uint32_t pk[NW];
#pragma unroll
        for (int k = 0; k < NW; ++k) pk[k] = 0;
#pragma unroll
        for (int i = 0; i < BPP; ++i) pk[i / 4] |= (uint32_t)res[i] << (8 * (i % 4));
#pragma unroll
        for (int k = 0; k < NW; ++k) { pk[k] = __shfl_up(pk[k], 1); if (lane == 0) pk[k] = 0; }
#pragma unroll
        for (int i = 0; i < BPP; ++i) {
          const int b = (pk[i / 4] >> (8 * (i % 4))) & 0xFF;
          const int a = u > 0 ? res[i] : 0, c = u > 0 ? bold[i] : 0;
          const int pred = ft == 0 ? 0 : ft == 1 ? a : ft == 2 ? b : ft == 3 ? (a + b) >> 1 : png_paeth(a, b, c);
          res[i] = (uint8_t)(raw[g][i] + pred);
          bold[i] = (uint8_t)b;
        }
        if (valid && !replay) {
          uint8_t* s = ring + lane * RS + (u & (RING - 1)) * KB;
          if constexpr (KB == 1) s[0] = res[0];  // grey (the high byte at depth 16), grey of grey + alpha, palette index
          else if constexpr (BPP == 3) { s[0] = res[0]; s[1] = res[1]; s[2] = res[2]; }
          else if constexpr (BPP == 4) {  // RGBA 8, or grey + alpha 16
            const bool rgba = ctype == 6;
            s[0] = res[0]; s[1] = rgba ? res[1] : res[0]; s[2] = rgba ? res[2] : res[0];
          } else { s[0] = res[0]; s[1] = res[2]; s[2] = res[4]; }  // RGB(A) 16: the high bytes
        }
        if (valid && saver) {
#pragma unroll
          for (int i = 0; i < BPP; ++i) save[(size_t)u * BPP + i] = res[i];
        }
      }
      // every lane has passed tile j once step 64 j + 126 is done; lane 0 enters tile j + 2 (the same ring slots) at 64 j + 128
      if ((t0 + G) % kPngTile == 0 && t0 + G >= 2 * kPngTile) {
        const int tile = (t0 + G) / kPngTile - 2;
        if (tile < ntiles) {
          __syncthreads();
          flush(tile);
          __syncthreads();
          flushed = tile + 1;
        }
      }
    }
    __syncthreads();
    for (; flushed < ntiles; ++flushed) flush(flushed);  // at most two tiles, none of them overwritten (64 (j + 2) >= U)
    __syncthreads();
    if (more) __threadfence();  // lane 63's reconstructed row, read by lane 0 of the next band
    first = next;
  }
}

}  // namespace

void launch_png(int kind, const PngImageDesc* imgs, const PngWork* work, int nwork, hipStream_t s) {
  if (nwork <= 0) return;
  const dim3 grid((unsigned)nwork), block(kPngBand);
  switch (kind) {
    case 0: hipLaunchKernelGGL(png_pixel_kernel<1>, grid, block, 0, s, imgs, work, nwork); break;
    case 1: hipLaunchKernelGGL(png_pixel_kernel<2>, grid, block, 0, s, imgs, work, nwork); break;
    case 2: hipLaunchKernelGGL(png_pixel_kernel<3>, grid, block, 0, s, imgs, work, nwork); break;
    case 3: hipLaunchKernelGGL(png_pixel_kernel<4>, grid, block, 0, s, imgs, work, nwork); break;
    case 4: hipLaunchKernelGGL(png_pixel_kernel<6>, grid, block, 0, s, imgs, work, nwork); break;
    case 5: hipLaunchKernelGGL(png_pixel_kernel<8>, grid, block, 0, s, imgs, work, nwork); break;
    default: break;
  }
}

}  // namespace ocr
