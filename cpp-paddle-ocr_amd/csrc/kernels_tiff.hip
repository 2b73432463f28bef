// The pixel half of the TIFF decoder on the device: expanded chunks (strips or tiles, chunky or in planes, 1 .. 16 bits a
// sample, differenced or not) -> packed BGR in the destination image, one launch per sample width a batch holds (the host
// keeps the container and what is serial: PackBits / LZW / Deflate, host/tiff_decode.h).
//
// The horizontal-differencing predictor stores every sample as the difference from the same sample of the pixel before it in
// the chunk's row: undoing it is a running sum per sample along the row - a scan, since addition modulo 2^8 / 2^16 is
// associative.  It is run as one:
//   - lanes run along the row.  A lane owns kTiffRun pixels, loads their samples and sums them per sample (up to four: the
//     colour samples and the alpha that premultiplies; extra samples behind them never reach a pixel and are not read)
//   - the run totals of a row's lanes are combined by a Hillis-Steele scan over the wave's lanes (ds_bpermute through
//     __shfl_up, log2(lanes of the row) steps); the four sums travel as 4 x 16 bits in one 64-bit value and are added
//     halfword by halfword, so a step is one shuffle whatever the sample count
//   - a row wider than one span of the wave (64 lanes x kTiffRun pixels) is walked span by span: the last lane's inclusive
//     sum is the carry into the next span.  No lane walks more than its own run of each span
//   - narrow chunk rows (16-pixel tiles, thin strips) are packed 64 / lanes_per_row to a wave: the scan is segmented by the
//     shuffle's width
//   - a wave is the unit of scheduling: the four waves of a workgroup take units of their own (no barrier, no LDS), and the
//     units of a launch - rows, chunks and the images of a batch - are walked with a grid stride
// The sums are exact integers modulo the sample width, so how a row is split into runs, spans or chunks cannot show.
//
// Loads and stores run along rows: neighbouring lanes read neighbouring bytes of a chunk's row (whatever the row's start or
// the pixel's size: bytes are fetched one by one or as the sample's two, never a byte outside the lane's pixels) and write
// neighbouring 12-byte groups of the output row - as three dwords where the row segment starts on a dword, bytewise where
// it does not (output rows start at any address: 3 * width bytes apart in a slot that packs images back to back) and for
// the ragged end of a row.
#include "kernels_tiff.h"

namespace ocr {
namespace {

#define TIFF_GLOBAL __attribute__((address_space(1)))
typedef const uint8_t TIFF_GLOBAL* TiffLoadPtr;
typedef uint8_t TIFF_GLOBAL* TiffBytePtr;

// 4 x 16-bit sums side by side, added halfword by halfword (no carry crosses a halfword)
__device__ __forceinline__ unsigned long long add4(unsigned long long a, unsigned long long b) {
  const unsigned long long low = 0x7FFF7FFF7FFF7FFFull;
  return ((a & low) + (b & low)) ^ ((a ^ b) & ~low);
}
__device__ __forceinline__ unsigned long long shuffle_up(unsigned long long v, int delta, int width) {
  const uint32_t lo = (uint32_t)__shfl_up((int)(uint32_t)v, delta, width), hi = (uint32_t)__shfl_up((int)(uint32_t)(v >> 32), delta, width);
  return ((unsigned long long)hi << 32) | lo;
}
__device__ __forceinline__ unsigned long long shuffle_from(unsigned long long v, int lane, int width) {
  const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)v, lane, width), hi = (uint32_t)__shfl((int)(uint32_t)(v >> 32), lane, width);
  return ((unsigned long long)hi << 32) | lo;
}

// one pixel from its samples v (v >> 16 k & 0xFFFF is sample k), as B | G << 8 | R << 16
__device__ __forceinline__ uint32_t tiff_convert(const TiffImageDesc& im, unsigned long long v) {
  const uint32_t s0 = (uint32_t)v & 0xFFFF, s1 = (uint32_t)(v >> 16) & 0xFFFF, s2 = (uint32_t)(v >> 32) & 0xFFFF, s3 = (uint32_t)(v >> 48);
  switch (im.mode) {
    case TIFF_PALETTE: return im.palette[s0 & 255];
    case TIFF_CMYK: {
      const uint32_t k = 255 - s3;
      return (k * (255 - s2) / 255) | ((k * (255 - s1) / 255) << 8) | ((k * (255 - s0) / 255) << 16);
    }
    case TIFF_GREY: {
      uint32_t c = im.bits == 16 ? s0 >> 8 : im.bits == 8 ? s0 : s0 * 255 / ((1u << im.bits) - 1);
      if (im.invert) c = 255 - c;
      return c * 0x010101u;
    }
    case TIFF_GREY_PLANES: {
      uint32_t c = s0, a = s1;
      if (im.bits == 16) { c = (c + 128) / 257; a = (a + 128) / 257; }
      if (im.premultiply) c = (c * a + 127) / 255;
      return c * 0x010101u;
    }
    default: {  // TIFF_RGB
      uint32_t r = s0, g = s1, b = s2, a = s3;
      if (im.bits == 16) { r = (r + 128) / 257; g = (g + 128) / 257; b = (b + 128) / 257; a = (a + 128) / 257; }
      if (im.premultiply) { r = (r * a + 127) / 255; g = (g * a + 127) / 255; b = (b * a + 127) / 255; }
      return b | (g << 8) | (r << 16);
    }
  }
}

// KIND 0: 1, 2, 4 bits (one sample, no predictor, chunky); 1: 8 bits; 2: 16 bits
template <int KIND>
__global__ void __launch_bounds__(kTiffBlock) tiff_pixel_kernel(const TiffImageDesc* __restrict__ imgs, int nimg, unsigned long long total_units) {
  const int lane = threadIdx.x & 63;
  const unsigned long long wave = (unsigned long long)blockIdx.x * kTiffWaves + (threadIdx.x >> 6), stride = (unsigned long long)gridDim.x * kTiffWaves;
  int f = 0;
  for (unsigned long long u = wave; u < total_units; u += stride) {  // (u, and all that follows from it alone, is uniform in the wave)
    while (f + 1 < nimg && imgs[f + 1].first_unit <= u) ++f;  // (units only grow: the search never goes back)
    const TiffImageDesc& im = imgs[f];
    const unsigned long long local = u - im.first_unit;
    const unsigned long long chunk = local / im.units_per_chunk;
    const int group = (int)(local % im.units_per_chunk);
    const int cy = (int)(chunk / (unsigned)im.across), cx = (int)(chunk % (unsigned)im.across);
    const int L = im.lanes_per_row, li = lane & (L - 1);
    const int yi = group * im.rows_per_unit + lane / L;
    const int cols = min(im.tile_width, im.width - cx * im.tile_width), rows = min(im.tile_height, im.height - cy * im.tile_height);
    const bool row_ok = yi < rows;
    const TiffLoadPtr src = (TiffLoadPtr)(uintptr_t)(im.data + (size_t)chunk * im.chunk_bytes + (size_t)(row_ok ? yi : 0) * im.row_bytes);
    uint8_t* out = im.bgr + (((size_t)cy * im.tile_height + (row_ok ? yi : 0)) * im.width + (size_t)cx * im.tile_width) * 3;
    const bool dwords = ((uintptr_t)out & 3) == 0;  // (a lane's group is 12 bytes behind its neighbour's: one answer for the row)
    const int spans = (cols + kTiffRun * L - 1) / (kTiffRun * L);  // more than one only when L is 64
    const int used = im.used, samples = im.samples;
    unsigned long long carry = 0;
    for (int s = 0; s < spans; ++s) {
      const int p = (s * L + li) * kTiffRun;
      const int n = row_ok ? max(0, min(kTiffRun, cols - p)) : 0;
      unsigned long long v[kTiffRun];
#pragma unroll
      for (int j = 0; j < kTiffRun; ++j) {
        v[j] = 0;
        if (j < n) {
          if constexpr (KIND == 0) {
            const int bits = im.bits, per = 8 / bits, x = p + j;
            v[j] = (src[x / per] >> ((per - 1 - x % per) * bits)) & ((1u << bits) - 1);
          } else {
            for (int k = 0; k < used; ++k) {
              constexpr int B = KIND;  // bytes of a sample
              const TiffLoadPtr q = im.plane_bytes ? src + (size_t)k * im.plane_bytes + (size_t)(p + j) * B : src + ((size_t)(p + j) * samples + k) * B;
              uint32_t t = q[0];
              if constexpr (KIND == 2) t = im.big_endian ? (t << 8) | q[1] : t | ((uint32_t)q[1] << 8);
              v[j] |= (unsigned long long)t << (16 * k);
            }
          }
        }
      }
      if (KIND != 0 && im.predictor == 2) {  // (uniform: every lane of the wave takes part in the shuffles)
#pragma unroll
        for (int j = 1; j < kTiffRun; ++j) v[j] = add4(v[j - 1], v[j]);  // the lane's run (pixels beyond n are zero: the total stands)
        unsigned long long total = v[kTiffRun - 1];
        for (int d = 1; d < L; d <<= 1) {
          const unsigned long long t = shuffle_up(total, d, L);
          if (li >= d) total = add4(total, t);
        }
        // total: the inclusive sum of the row's lanes up to this one; what comes in front of the lane's run is that without its own
        unsigned long long before = shuffle_up(total, 1, L);
        before = li == 0 ? carry : add4(before, carry);
        carry = add4(shuffle_from(total, L - 1, L), carry);
#pragma unroll
        for (int j = 0; j < kTiffRun; ++j) v[j] = add4(v[j], before);
        if constexpr (KIND == 1) {
#pragma unroll
          for (int j = 0; j < kTiffRun; ++j) v[j] &= 0x00FF00FF00FF00FFull;  // the sum of bytes is a byte
        }
      }
      if (n > 0) {
        uint32_t c[kTiffRun];
#pragma unroll
        for (int j = 0; j < kTiffRun; ++j) c[j] = tiff_convert(im, v[j]);
        const TiffBytePtr o = (TiffBytePtr)(uintptr_t)(out + (size_t)p * 3);
        if (n == kTiffRun && dwords) {
          uint32_t TIFF_GLOBAL* o32 = (uint32_t TIFF_GLOBAL*)o;  // adjacent dwords: one global_store_dwordx3
          o32[0] = c[0] | (c[1] << 24);
          o32[1] = (c[1] >> 8) | (c[2] << 16);
          o32[2] = (c[2] >> 16) | (c[3] << 8);
        } else {
          for (int j = 0; j < n; ++j) { o[3 * j] = (uint8_t)c[j]; o[3 * j + 1] = (uint8_t)(c[j] >> 8); o[3 * j + 2] = (uint8_t)(c[j] >> 16); }
        }
      }
    }
  }
}

template <int KIND> void tiff_launch_kind(const TiffImageDesc* imgs, int nimg, unsigned long long total, hipStream_t s) {
  const unsigned long long groups = (total + kTiffWaves - 1) / kTiffWaves;
  const dim3 grid((unsigned)(groups < (unsigned long long)kTiffMaxGrid ? groups : (unsigned long long)kTiffMaxGrid)), block(kTiffBlock);
  hipLaunchKernelGGL(tiff_pixel_kernel<KIND>, grid, block, 0, s, imgs, nimg, total);
}

// the yardstick of decode_tool --time: a plain copy, 16 bytes a lane, grid stride
__global__ void __launch_bounds__(kTiffBlock) plain_copy_kernel(const uint4* __restrict__ src, uint4* __restrict__ dst, size_t n) {
  for (size_t i = (size_t)blockIdx.x * kTiffBlock + threadIdx.x; i < n; i += (size_t)gridDim.x * kTiffBlock) dst[i] = src[i];
}

}  // namespace

void launch_plain_copy(void* dst, const void* src, size_t bytes, hipStream_t s) {
  const size_t n = bytes / 16, groups = (n + kTiffBlock - 1) / kTiffBlock;
  if (n == 0) return;
  hipLaunchKernelGGL(plain_copy_kernel, dim3((unsigned)(groups < (size_t)(4 * kTiffMaxGrid) ? groups : (size_t)(4 * kTiffMaxGrid))), dim3(kTiffBlock), 0, s,
                     (const uint4*)src, (uint4*)dst, n);
}

void launch_tiff(int kind, const TiffImageDesc* imgs, int nimg, unsigned long long total_units, hipStream_t s) {
  if (nimg <= 0 || total_units == 0) return;
  switch (kind) {
    case 0: tiff_launch_kind<0>(imgs, nimg, total_units, s); break;
    case 1: tiff_launch_kind<1>(imgs, nimg, total_units, s); break;
    case 2: tiff_launch_kind<2>(imgs, nimg, total_units, s); break;
    default: break;
  }
}

}  // namespace ocr
