// The pixel half of the BMP / PNM decoders on the device: stored rows (1 / 4 / 8-bit indices, 5-5-5 / 5-6-5, BGR, BGRX,
// RGB, grey, big-endian 16-bit samples, PBM bits) -> packed BGR, one launch per kind a batch holds (the host keeps the
// containers and what is serial: run-length expansion and ASCII parsing, host/raw_decode.h).
//
// A pure streaming kernel, bound by its stores: 3 output bytes for every 1/8 .. 6 input bytes.  So the shape is set by the
// loads and stores:
//   - a workgroup owns a span of ONE output row (kRawBlock lanes x 4 pixels); bottom_up only changes which stored row it
//     reads - an index, never a second pass.  The units of a launch are walked with a grid stride; which frame, row and
//     span a unit is depends on blockIdx alone, so the descriptor table is read with scalar loads
//   - output rows start at any address (a row is 3 * width bytes into a slot that packs images back to back).  The row's
//     first h = (address & 3) pixels are its head: pixel h starts on a dword (3 h = -h mod 4), and every group of 4 pixels
//     behind it is three whole dwords.  A lane writes its group as those three dwords; the head (lanes 0 .. h-1 of span 0)
//     and a last group of fewer than 4 pixels are written bytewise
//   - a lane's 4 pixels are 1 .. 24 consecutive stored bytes at any alignment (BGR24 at odd widths, P4 / P6 rows without
//     padding, the head's shift): they are fetched as the whole dwords that cover them - never a byte outside those - and
//     brought into place with v_alignbyte
//   - the palette of the INDEX kinds is fetched once per workgroup (again when the grid stride crosses into another
//     frame) into LDS as 256 packed dwords; a lookup is one ds_read_b32
#include "kernels_raw.h"

namespace ocr {
namespace {

// The data and output pointers come out of the descriptor table, where the compiler cannot see their address space; said
// to be global, the accesses are global_load / global_store, not flat ones.
#define RAW_GLOBAL __attribute__((address_space(1)))
typedef const uint32_t RAW_GLOBAL* RawLoadPtr;
typedef uint8_t RAW_GLOBAL* RawBytePtr;

enum { INDEX1, INDEX4, INDEX8, BGR555, BGR565, BGR24, BGRX32, RGB24, GREY8, GREY16BE, RGB48BE, BIT1_INV };

template <int KIND> struct RawTraits {
  static constexpr bool kBits = KIND == INDEX1 || KIND == BIT1_INV, kNibbles = KIND == INDEX4;
  static constexpr bool kIndexed = KIND == INDEX1 || KIND == INDEX4 || KIND == INDEX8;
  // bytes per pixel of the byte-addressed kinds
  static constexpr int kBpp = KIND == INDEX8 || KIND == GREY8 ? 1 : KIND == BGR555 || KIND == BGR565 || KIND == GREY16BE ? 2
                            : KIND == BGR24 || KIND == RGB24 ? 3 : KIND == BGRX32 ? 4 : KIND == RGB48BE ? 6 : 0;
  // the most stored bytes 4 pixels touch (bits: 2 bytes when they straddle one; nibbles: 3 from an odd pixel)
  static constexpr int kMaxBytes = kBits ? 2 : kNibbles ? 3 : kBpp * kRawGroup;
  static constexpr int kWords = (kMaxBytes + 3) / 4;
};

// byte j of the fetched bytes
template <int NW> __device__ __forceinline__ uint32_t raw_byte(const uint32_t (&w)[NW], int j) { return (w[j >> 2] >> (8 * (j & 3))) & 0xFF; }

// bytes [p, p + nb) of device memory, nb <= 4 NW, into w as little-endian words: the aligned dwords that hold them, no other
template <int NW> __device__ __forceinline__ void raw_fetch(const uint8_t* p, int nb, uint32_t (&w)[NW]) {
  const uintptr_t a = (uintptr_t)p;
  const RawLoadPtr q = (RawLoadPtr)(a & ~(uintptr_t)3);
  const int sh = (int)(a & 3);
  uint32_t d[NW + 1];
#pragma unroll
  for (int k = 0; k <= NW; ++k) d[k] = 4 * k < sh + nb ? q[k] : 0u;
#pragma unroll
  for (int k = 0; k < NW; ++k) w[k] = __builtin_amdgcn_alignbyte(d[k + 1], d[k], (uint32_t)sh);
}

// pixels [p, p + n) of the stored row `src` (n <= 4) as packed B | G << 8 | R << 16
template <int KIND> __device__ __forceinline__ void raw_convert(const uint8_t* src, int p, int n, const uint32_t* pal, uint32_t (&c)[kRawGroup]) {
  using T = RawTraits<KIND>;
  uint32_t w[T::kWords];
  if constexpr (T::kBits) {
    const int b0 = p >> 3;
    raw_fetch<T::kWords>(src + b0, ((p + n - 1) >> 3) - b0 + 1, w);
#pragma unroll
    for (int i = 0; i < kRawGroup; ++i) {
      const int bit = (p & 7) + i;  // from the most significant bit of byte b0
      const uint32_t v = (w[0] >> (8 * (bit >> 3) + 7 - (bit & 7))) & 1;
      c[i] = KIND == INDEX1 ? pal[v] : v ? 0u : 0xFFFFFFu;
    }
  } else if constexpr (T::kNibbles) {
    const int b0 = p >> 1;
    raw_fetch<T::kWords>(src + b0, ((p + n - 1) >> 1) - b0 + 1, w);
#pragma unroll
    for (int i = 0; i < kRawGroup; ++i) {
      const int nib = (p & 1) + i;  // from the high nibble of byte b0
      c[i] = pal[(w[0] >> (8 * (nib >> 1) + ((nib & 1) ? 0 : 4))) & 15];
    }
  } else {
    raw_fetch<T::kWords>(src + (size_t)p * T::kBpp, n * T::kBpp, w);
#pragma unroll
    for (int i = 0; i < kRawGroup; ++i) {
      constexpr int B = T::kBpp;
      if constexpr (KIND == INDEX8) c[i] = pal[raw_byte(w, i)];
      else if constexpr (KIND == GREY8) c[i] = raw_byte(w, i) * 0x010101u;
      else if constexpr (KIND == GREY16BE) c[i] = raw_byte(w, B * i) * 0x010101u;  // the high byte comes first
      else if constexpr (KIND == BGR555) { const uint32_t t = raw_byte(w, B * i) | (raw_byte(w, B * i + 1) << 8); c[i] = ((t << 3) & 0xFF) | (((t >> 2) & 0xF8) << 8) | (((t >> 7) & 0xF8) << 16); }
      else if constexpr (KIND == BGR565) { const uint32_t t = raw_byte(w, B * i) | (raw_byte(w, B * i + 1) << 8); c[i] = ((t << 3) & 0xFF) | (((t >> 3) & 0xFC) << 8) | (((t >> 8) & 0xF8) << 16); }
      else if constexpr (KIND == BGR24 || KIND == BGRX32) c[i] = raw_byte(w, B * i) | (raw_byte(w, B * i + 1) << 8) | (raw_byte(w, B * i + 2) << 16);
      else if constexpr (KIND == RGB24) c[i] = raw_byte(w, B * i + 2) | (raw_byte(w, B * i + 1) << 8) | (raw_byte(w, B * i) << 16);
      else c[i] = raw_byte(w, B * i + 4) | (raw_byte(w, B * i + 2) << 8) | (raw_byte(w, B * i) << 16);  // RGB48BE: the high bytes
    }
  }
}

template <int KIND>
__global__ void __launch_bounds__(kRawBlock) raw_pixel_kernel(const RawImageDesc* __restrict__ imgs, int nimg, unsigned long long total_units) {
  __shared__ uint32_t pal[256];
  const int lane = threadIdx.x;
  int f = 0, loaded = -1;
  for (unsigned long long u = blockIdx.x; u < total_units; u += gridDim.x) {
    while (f + 1 < nimg && imgs[f + 1].first_unit <= u) ++f;  // (units only grow: the search never goes back)
    const RawImageDesc& im = imgs[f];
    if constexpr (RawTraits<KIND>::kIndexed) {
      if (loaded != f) {
        if (loaded >= 0) __syncthreads();  // the lanes still reading the palette before
        pal[lane] = im.palette[lane];
        __syncthreads();
        loaded = f;
      }
    }
    const unsigned local = (unsigned)(u - im.first_unit), spans = im.spans;
    const int y = (int)(local / spans), span = (int)(local % spans);
    const int width = im.width;
    const uint8_t* src = im.data + (size_t)(im.bottom_up ? im.height - 1 - y : y) * im.row_stride;
    uint8_t* out = im.bgr + (size_t)y * width * 3;
    const int head = min((int)((uintptr_t)out & 3), width);
    uint32_t c[kRawGroup];
    // the groups of this span
    const long long p64 = (long long)head + ((long long)span * kRawBlock + lane) * kRawGroup;
    if (p64 < width) {
      const int p = (int)p64, n = min(kRawGroup, width - p);
      raw_convert<KIND>(src, p, n, pal, c);
      const RawBytePtr o = (RawBytePtr)(uintptr_t)(out + (size_t)p * 3);
      if (n == kRawGroup) {
        uint32_t RAW_GLOBAL* o32 = (uint32_t RAW_GLOBAL*)o;  // adjacent dwords: one global_store_dwordx3
        o32[0] = c[0] | (c[1] << 24);
        o32[1] = (c[1] >> 8) | (c[2] << 16);
        o32[2] = (c[2] >> 16) | (c[3] << 8);
      } else {
        for (int i = 0; i < n; ++i) { o[3 * i] = (uint8_t)c[i]; o[3 * i + 1] = (uint8_t)(c[i] >> 8); o[3 * i + 2] = (uint8_t)(c[i] >> 16); }
      }
    }
    // the row's head: pixels in front of the first aligned dword
    if (span == 0 && lane < head) {
      raw_convert<KIND>(src, lane, 1, pal, c);
      const RawBytePtr o = (RawBytePtr)(uintptr_t)(out + (size_t)lane * 3);
      o[0] = (uint8_t)c[0]; o[1] = (uint8_t)(c[0] >> 8); o[2] = (uint8_t)(c[0] >> 16);
    }
  }
}

template <int KIND> void raw_launch_kind(const RawImageDesc* imgs, int nimg, unsigned long long total, hipStream_t s) {
  const dim3 grid((unsigned)(total < (unsigned long long)kRawMaxGrid ? total : (unsigned long long)kRawMaxGrid)), block(kRawBlock);
  hipLaunchKernelGGL(raw_pixel_kernel<KIND>, grid, block, 0, s, imgs, nimg, total);
}

}  // namespace

void launch_raw(int kind, const RawImageDesc* imgs, int nimg, unsigned long long total_units, hipStream_t s) {
  if (nimg <= 0 || total_units == 0) return;
  switch (kind) {
    case INDEX1: raw_launch_kind<INDEX1>(imgs, nimg, total_units, s); break;
    case INDEX4: raw_launch_kind<INDEX4>(imgs, nimg, total_units, s); break;
    case INDEX8: raw_launch_kind<INDEX8>(imgs, nimg, total_units, s); break;
    case BGR555: raw_launch_kind<BGR555>(imgs, nimg, total_units, s); break;
    case BGR565: raw_launch_kind<BGR565>(imgs, nimg, total_units, s); break;
    case BGR24: raw_launch_kind<BGR24>(imgs, nimg, total_units, s); break;
    case BGRX32: raw_launch_kind<BGRX32>(imgs, nimg, total_units, s); break;
    case RGB24: raw_launch_kind<RGB24>(imgs, nimg, total_units, s); break;
    case GREY8: raw_launch_kind<GREY8>(imgs, nimg, total_units, s); break;
    case GREY16BE: raw_launch_kind<GREY16BE>(imgs, nimg, total_units, s); break;
    case RGB48BE: raw_launch_kind<RGB48BE>(imgs, nimg, total_units, s); break;
    case BIT1_INV: raw_launch_kind<BIT1_INV>(imgs, nimg, total_units, s); break;
    default: break;
  }
}

}  // namespace ocr
