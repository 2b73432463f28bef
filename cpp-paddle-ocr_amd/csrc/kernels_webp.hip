// The pixel half of the lossless WebP decoder on the device: the entropy-decoded ARGB image and the transforms' sub-images ->
// packed BGR in the destination image (the host keeps the container and what is serial: prefix codes, LZ77, the colour cache,
// host/webp_decode.h).  Two kernels, one launch each per batch.
//
// WITH A PREDICTOR (webp_predict_kernel).  Undoing the spatial predictor is a dependency chain of the PNG kind - a pixel
// needs L, T, TL and, unlike PNG, TR - and Select and the clamped modes are not associative: no scan.  What is parallel is the
// anti-diagonal of a block of rows and the images of a batch.
//   - a workgroup is ONE wave and takes one image; it walks it in bands of 64 rows, lane l owning row r0 + l
//   - the skew is TWO pixels a lane: at step t lane l reconstructs pixel x = t - 2 l.  TR of x is pixel x + 1 of the row
//     above, which the lane above finished one step ago.  So one one-lane shuffle a step - of every lane's last result -
//     delivers TR; T is the TR of the step before and TL the T of the step before: registers only.  L is the lane's own last
//     result.  TR of the row's last pixel is the row's own pixel 0, which the lane keeps
//   - a pixel is one dword; the four channels are done with packed byte arithmetic (no carry crosses a byte): sums as two
//     masked halves, averages as (a & b) + (((a ^ b) & 0xfefefefe) >> 1), the Select distance with v_sad_u8
//   - the block's mode is fetched when the lane enters the block, not per pixel; pixel (0, 0), the top row and the left
//     column have their fixed modes
//   - pointwise transforms that are undone BEFORE the predictor (cross-colour in every file of libwebp's encoder) are applied
//     to the residual as it is loaded, its multipliers fetched per block; those undone AFTER it (add-green, the palette
//     lookup with bit unbundling) are applied at flush time
//   - bands after the first take 63 new rows: lane 0 REPLAYS the last row of the band before, which that band's last lane
//     wrote, reconstructed, to `recon` (the only intermediate bytes that reach memory; a row of its own per band, so no
//     line is read before it was written), and feeds lane 1 as any row above would
//   - the residual loads of 8 steps are issued together ahead of the 8 dependent steps
//   - at any step the 64 lanes sit in 64 different rows, so a store per lane would be 3 bytes to each of 64 lines.  Finished
//     pixels go to an LDS ring of 64 rows instead and are written out tile by tile (64 coded pixels of every row), lanes
//     along the row: contiguous BGR bytes.  The front spans 2 * 63 + 1 = 127 pixels, so tile j is complete after step
//     64 j + 63 + 126 = 64 j + 189: it is flushed at the boundary 64 (j + 3), and lane 0 enters tile j + 3 at that very step -
//     the ring holds THREE tiles (192 pixels; two, as PNG has, would be overwritten before they are whole).
//     A ring row is 192 + 3 dwords.  Derivation: lane l writes dword l * RS + (t - 2 l) mod 192, so the front advances by
//     RS - 2 dwords per lane (the ring's wrap subtracts 192, a multiple of the 32 banks a ds_write_b32 is banked over, in
//     32-lane halves).  RS - 2 = 193 = 1 mod 32: the 32 lanes of a half write 32 different banks.  The flush reads
//     consecutive dwords of one ring row: one bank per lane as well.
// WITHOUT ONE (webp_stream_kernel): palette-only, add-green-only and cross-colour-only files (and their combinations) are a
// pure streaming job shaped like raw_pixel_kernel: a workgroup owns a span of ONE output row, the units of a launch are
// walked with a grid stride and found from blockIdx alone (the descriptor table is read with scalar loads), the palette sits
// in LDS as 256 packed dwords, and a lane writes its 4 pixels as three aligned dwords - the row's head in front of the
// first aligned dword and a last group of fewer than 4 pixels bytewise.
#include "kernels_webp.h"

namespace ocr {
namespace {

#define WEBP_GLOBAL __attribute__((address_space(1)))
typedef const uint32_t WEBP_GLOBAL* WebpLoadPtr;
typedef uint32_t WEBP_GLOBAL* WebpWordPtr;
typedef uint8_t WEBP_GLOBAL* WebpBytePtr;

__device__ __forceinline__ uint32_t add_bytes(uint32_t a, uint32_t b) {
  return (((a & 0xFF00FF00u) + (b & 0xFF00FF00u)) & 0xFF00FF00u) | (((a & 0x00FF00FFu) + (b & 0x00FF00FFu)) & 0x00FF00FFu);
}
__device__ __forceinline__ uint32_t avg2(uint32_t a, uint32_t b) { return (a & b) + (((a ^ b) & 0xFEFEFEFEu) >> 1); }
__device__ __forceinline__ uint32_t clamp_full(uint32_t L, uint32_t T, uint32_t TL) {
  uint32_t r = 0;
#pragma unroll
  for (int s = 0; s < 32; s += 8) {
    const int v = (int)((L >> s) & 255) + (int)((T >> s) & 255) - (int)((TL >> s) & 255);
    r |= (uint32_t)min(max(v, 0), 255) << s;
  }
  return r;
}
__device__ __forceinline__ uint32_t clamp_half(uint32_t L, uint32_t T, uint32_t TL) {
  const uint32_t a = avg2(L, T);
  uint32_t r = 0;
#pragma unroll
  for (int s = 0; s < 32; s += 8) {
    const int x = (int)((a >> s) & 255), y = (int)((TL >> s) & 255);
    r |= (uint32_t)min(max(x + (x - y) / 2, 0), 255) << s;  // C's division: towards zero
  }
  return r;
}
__device__ __forceinline__ uint32_t webp_predict(int mode, uint32_t L, uint32_t T, uint32_t TL, uint32_t TR) {
  switch (mode) {
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
    case 11:  // Select: T when |L - TL| summed over the channels is at most |T - TL|
      return __builtin_amdgcn_sad_u8(L, TL, 0u) <= __builtin_amdgcn_sad_u8(T, TL, 0u) ? T : L;
    case 12: return clamp_full(L, T, TL);
    case 13: return clamp_half(L, T, TL);
    default: return 0xFF000000u;  // 0, 14, 15
  }
}
__device__ __forceinline__ uint32_t cross_colour(uint32_t v, uint32_t m) {
  const int g2r = (int8_t)(m & 255), g2b = (int8_t)((m >> 8) & 255), r2b = (int8_t)((m >> 16) & 255);
  const int green = (int8_t)((v >> 8) & 255);
  const uint32_t red = ((v >> 16) + (uint32_t)((g2r * green) >> 5)) & 255;
  uint32_t blue = v + (uint32_t)((g2b * green) >> 5);
  blue = (blue + (uint32_t)((r2b * (int)(int8_t)red) >> 5)) & 255;
  return (v & 0xFF00FF00u) | (red << 16) | blue;
}
__device__ __forceinline__ uint32_t add_green(uint32_t v) {
  const uint32_t g = (v >> 8) & 255;
  return (v & 0xFF00FF00u) | (((v & 0x00FF00FFu) + (g << 16 | g)) & 0x00FF00FFu);
}
// the multipliers of coded pixel (c, y)
__device__ __forceinline__ uint32_t cross_at(const WebpImageDesc& im, int y, int c) {
  const int bw = (im.coded_width + (1 << im.cross_bits) - 1) >> im.cross_bits;
  return ((WebpLoadPtr)(uintptr_t)im.cross)[(size_t)(y >> im.cross_bits) * bw + (c >> im.cross_bits)];
}
__device__ __forceinline__ uint32_t apply_ops(const WebpImageDesc& im, int n, const int (&ops)[2], uint32_t v, int y, int c) {
  for (int k = 0; k < n; ++k) v = ops[k] == WEBP_OP_CROSS ? cross_colour(v, cross_at(im, y, c)) : add_green(v);
  return v;
}
__device__ __forceinline__ void put_bgr(uint8_t* out, uint32_t v) {
  const WebpBytePtr o = (WebpBytePtr)(uintptr_t)out;
  o[0] = (uint8_t)v; o[1] = (uint8_t)(v >> 8); o[2] = (uint8_t)(v >> 16);
}

__global__ void __launch_bounds__(kWebpBand) webp_predict_kernel(const WebpImageDesc* __restrict__ imgs, int nimg) {
  constexpr int RS = kWebpRing + 3;  // dwords per ring row
  constexpr int G = 8;               // steps per group of loads (divides kWebpTile)
  __shared__ uint32_t ring[kWebpBand * RS];
  __shared__ uint32_t pal[256];
  if ((int)blockIdx.x >= nimg) return;
  const WebpImageDesc& im = imgs[blockIdx.x];
  const int lane = threadIdx.x;
  const int W = im.coded_width, H = im.height, width = im.width;
  const int pbits = im.pred_bits, pmask = (1 << pbits) - 1, pbw = (W + pmask) >> pbits;
  const int ibits = im.index_bits;
  const int npre = im.npre, npost = im.npost;
  const int pre[2] = {im.pre[0], im.pre[1]}, post[2] = {im.post[0], im.post[1]};
  const int xmask = (1 << im.cross_bits) - 1;
  const bool pre_cross = (npre > 0 && pre[0] == WEBP_OP_CROSS) || (npre > 1 && pre[1] == WEBP_OP_CROSS);
  const WebpLoadPtr argb = (WebpLoadPtr)(uintptr_t)im.argb, modes = (WebpLoadPtr)(uintptr_t)im.pred;
  const int ntiles = (W + kWebpTile - 1) / kWebpTile;
  if (ibits >= 0) {
    for (int k = lane; k < 256; k += kWebpBand) pal[k] = im.palette[k];
  }
  __syncthreads();

  for (int first = 0, band = 0; first < H; ++band) {
    const int row0 = band == 0 ? 0 : first - 1;  // lane 0's row: the image's first, or the replayed one
    const int nl = min(kWebpBand, H - row0);
    const int next = row0 + nl;
    const bool more = next < H;                  // (then nl == kWebpBand)
    const bool active = lane < nl, replay = band > 0 && lane == 0, saver = more && lane == nl - 1;
    const int y = active ? row0 + lane : 0;
    const WebpLoadPtr src = replay ? (WebpLoadPtr)(uintptr_t)im.recon + (size_t)(band - 1) * W : argb + (size_t)y * W;
    const WebpWordPtr save = (WebpWordPtr)(uintptr_t)im.recon + (size_t)band * W;  // (written by the saver alone: there is such a row then)
    const WebpLoadPtr mrow = modes + (size_t)(y >> pbits) * pbw;

    // tile j of the ring -> the image, row by row (uniform: every lane calls it)
    auto flush = [&](int tile) {
      const int c = tile * kWebpTile + lane;
      for (int r = band > 0 ? 1 : 0; r < nl; ++r) {
        if (c >= W) continue;
        const int yr = row0 + r;
        uint32_t v = ring[r * RS + c % kWebpRing];
        v = apply_ops(im, npost, post, v, yr, c);
        uint8_t* orow = im.bgr + (size_t)yr * width * 3;
        if (ibits < 0) {
          put_bgr(orow + (size_t)c * 3, v);
        } else {
          const int per = 1 << ibits, each = 8 >> ibits;
          const uint32_t packed = (v >> 8) & 255;
          for (int k = 0; k < per; ++k) {
            const int xo = (c << ibits) + k;
            if (xo < width) put_bgr(orow + (size_t)xo * 3, pal[(packed >> (k * each)) & ((1u << each) - 1)]);
          }
        }
      }
    };

    uint32_t last = 0, tr = 0, t_ = 0, tl = 0, row_first = 0, mode_word = 0, mult = 0;
    const int nsteps = W + 2 * (nl - 1);
    for (int t0 = 0; t0 < nsteps; t0 += G) {
      uint32_t raw[G];
#pragma unroll
      for (int g = 0; g < G; ++g) {
        const int x = t0 + g - 2 * lane;
        raw[g] = active && x >= 0 && x < W ? src[x] : 0u;
      }
#pragma unroll
      for (int g = 0; g < G; ++g) {
        const int x = t0 + g - 2 * lane;
        const bool valid = active && x >= 0 && x < W;
        // what the lane above finished one step ago is this pixel's TR; its T and TL arrived the same way one and two steps ago
        tl = t_;
        t_ = tr;
        tr = (uint32_t)__shfl_up((int)last, 1);
        if (valid) {
          uint32_t v = raw[g];
          if (!replay) {
            if ((x & pmask) == 0) mode_word = mrow[x >> pbits];
            if (pre_cross && (x & xmask) == 0) mult = cross_at(im, y, x);
            for (int k = 0; k < npre; ++k) v = pre[k] == WEBP_OP_CROSS ? cross_colour(v, mult) : add_green(v);
            const int mode = y == 0 ? (x == 0 ? 0 : 1) : x == 0 ? 2 : (int)((mode_word >> 8) & 15);
            v = add_bytes(v, webp_predict(mode, last, t_, tl, x == W - 1 ? row_first : tr));
            ring[lane * RS + x % kWebpRing] = v;
          }
          if (x == 0) row_first = v;
          last = v;
          if (saver) save[x] = v;
        }
      }
      // every lane has passed tile j once step 64 j + 189 is done; lane 0 enters tile j + 3 (the same ring slots) at 64 j + 192
      if ((t0 + G) % kWebpTile == 0 && t0 + G >= 3 * kWebpTile) {
        const int tile = (t0 + G) / kWebpTile - 3;
        if (tile < ntiles) {
          __syncthreads();
          flush(tile);
          __syncthreads();
        }
      }
    }
    __syncthreads();
    {
      // the tiles no boundary of the loop reached: at most three, none of them overwritten (64 (j + 3) > the steps done)
      const int done = (nsteps + G - 1) / G * G / kWebpTile - 2;  // tiles flushed in the loop: those with 64 (j + 3) <= steps run
      for (int tile = max(done, 0); tile < ntiles; ++tile) flush(tile);
    }
    __syncthreads();
    if (more) __threadfence();  // the last lane's reconstructed row, read by lane 0 of the next band
    first = next;
  }
}

// the BGR dword of output pixel (xo, y) of a frame without a predictor
__device__ __forceinline__ uint32_t stream_pixel(const WebpImageDesc& im, const uint32_t* pal, int y, int xo) {
  const int ibits = im.index_bits;
  const int c = ibits > 0 ? xo >> ibits : xo;
  uint32_t v = ((WebpLoadPtr)(uintptr_t)im.argb)[(size_t)y * im.coded_width + c];
  v = apply_ops(im, im.npre, im.pre, v, y, c);
  if (ibits < 0) return v;
  const int each = 8 >> ibits;
  return pal[(((v >> 8) & 255) >> ((xo & ((1 << ibits) - 1)) * each)) & ((1u << each) - 1)];
}

__global__ void __launch_bounds__(kWebpBlock) webp_stream_kernel(const WebpImageDesc* __restrict__ imgs, int nimg, unsigned long long total_units) {
  __shared__ uint32_t pal[256];
  const int lane = threadIdx.x;
  int f = 0, loaded = -1;
  for (unsigned long long u = blockIdx.x; u < total_units; u += gridDim.x) {
    while (f + 1 < nimg && imgs[f + 1].first_unit <= u) ++f;  // (units only grow: the search never goes back)
    const WebpImageDesc& im = imgs[f];
    if (loaded != f) {
      if (loaded >= 0) __syncthreads();  // the lanes still reading the palette before
      pal[lane] = im.palette[lane];
      __syncthreads();
      loaded = f;
    }
    const unsigned local = (unsigned)(u - im.first_unit), spans = im.spans;
    const int y = (int)(local / spans), span = (int)(local % spans);
    const int width = im.width;
    uint8_t* out = im.bgr + (size_t)y * width * 3;
    const int head = min((int)((uintptr_t)out & 3), width);
    const long long p64 = (long long)head + ((long long)span * kWebpBlock + lane) * kWebpGroup;
    if (p64 < width) {
      const int p = (int)p64, n = min(kWebpGroup, width - p);
      uint32_t c[kWebpGroup];
#pragma unroll
      for (int i = 0; i < kWebpGroup; ++i) c[i] = i < n ? stream_pixel(im, pal, y, p + i) & 0xFFFFFFu : 0u;
      if (n == kWebpGroup) {
        uint32_t WEBP_GLOBAL* o32 = (uint32_t WEBP_GLOBAL*)(uintptr_t)(out + (size_t)p * 3);  // adjacent dwords: one global_store_dwordx3
        o32[0] = c[0] | (c[1] << 24);
        o32[1] = (c[1] >> 8) | (c[2] << 16);
        o32[2] = (c[2] >> 16) | (c[3] << 8);
      } else {
        for (int i = 0; i < n; ++i) put_bgr(out + (size_t)(p + i) * 3, c[i]);
      }
    }
    // the row's head: pixels in front of the first aligned dword
    if (span == 0 && lane < head) put_bgr(out + (size_t)lane * 3, stream_pixel(im, pal, y, lane));
  }
}

}  // namespace

void launch_webp(int kind, const WebpImageDesc* imgs, int nimg, unsigned long long total_units, hipStream_t s) {
  if (nimg <= 0) return;
  if (kind == 0) {
    hipLaunchKernelGGL(webp_predict_kernel, dim3((unsigned)nimg), dim3(kWebpBand), 0, s, imgs, nimg);
  } else if (total_units > 0) {
    const dim3 grid((unsigned)(total_units < (unsigned long long)kWebpMaxGrid ? total_units : (unsigned long long)kWebpMaxGrid));
    hipLaunchKernelGGL(webp_stream_kernel, grid, dim3(kWebpBlock), 0, s, imgs, nimg, total_units);
  }
}

}  // namespace ocr
