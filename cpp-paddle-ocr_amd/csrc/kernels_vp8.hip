// The pixel half of the lossy WebP (VP8 key frame) decoder on the device.  The arithmetic - transforms, sub-block
// predictors, filters, upsampling, colour conversion - is host/vp8_decode.h's, compiled for the device; what is here is how the
// work is laid out.
//
// vp8_recon_kernel: one workgroup of kVp8Waves waves per image.  Macroblock (x, y) needs the unfiltered pixels of its left, top
// and top-right neighbours, so all macroblocks with the same x + 2 y are independent: the workgroup walks these diagonals in
// order, a wave owns a macroblock of the diagonal (wave w takes the w-th, (w + kVp8Waves)-th ... row of it), and a workgroup
// barrier separates the diagonals.  No wave waits for another workgroup: there is nothing to spin on.  A wave keeps its
// macroblock in LDS in the host's work-area layout (stride 32, the neighbours around it): coefficients are scattered from the
// compact array, 16x16 and chroma prediction take 4 pixels a lane, the inverse transforms a block a lane, and a B_PRED
// macroblock's 16 sub-blocks - each needs the pixels of the one before - run in raster order on lane 0.  The planes are
// written unfiltered; prediction never sees a filtered pixel because the filter is a launch of its own.
// vp8_filter_kernel: the same walk (filtering (x, y) changes up to three pixels of its left and top neighbours and reads a
// fourth, and (x + 1, y - 1) changes the top neighbour's right-most columns first).  Left edge and inner vertical edges: a
// lane owns a row (16 luma, 8 + 8 chroma) and goes over its edges in order; then top edge and inner horizontal edges with a
// lane a column.
// vp8_convert_kernel: a lane makes kVp8Group consecutive pixels of the packed output - the image taken as one run of
// pixels, so that a lane's 12 bytes start on a dword whatever the width: unit 0 is the (bgr & 3) pixels in front of the
// first aligned one and is stored bytewise, as is the last, short unit; every other unit is three dword stores.
//
// Known slack, kept for a layout that is easy to check: the phases of a macroblock are separated by workgroup barriers although
// the LDS areas are a wave's own (only the barrier behind a diagonal needs the whole group; the others keep every wave on the same
// trip count); a B_PRED macroblock occupies one lane while 63 wait (the four sub-blocks of an anti-diagonal of the 4 x 4 grid
// could share lanes); the filter uses 32 of a wave's 64 lanes.  One image is therefore latency-bound and loses to a host
// thread; a batch wins by the images in flight (profiles/webp_lossy_pixel_stage.json).
#include "kernels_vp8.h"

namespace ocr {

namespace {

using namespace PaddleOCR::vp8;
using namespace PaddleOCR::vp8::detail;

constexpr int kYArea = kBps * 17 + 8, kCArea = kBps * 9 + 8;

// the rows of diagonal d: y in [lo, hi], x = d - 2 y
__device__ inline void diagonal(int d, int mw, int mh, int& lo, int& hi) {
  lo = d - mw + 1 > 0 ? (d - mw + 2) >> 1 : 0;
  hi = d >> 1 < mh - 1 ? d >> 1 : mh - 1;
}

// pixel (x, y) of a size x size block predicted in `mode` (16x16 luma and chroma), d: the block in its work area
__device__ inline int predict_px(int mode, const uint8_t* d, int size, bool has_top, bool has_left, int x, int y) {
  const uint8_t* top = d - kBps;
  if (mode == V_PRED) return top[x];
  if (mode == H_PRED) return d[-1 + y * kBps];
  if (mode == TM_PRED) return clip8(top[x] + d[-1 + y * kBps] - top[-1]);
  if (!has_top && !has_left) return 0x80;
  int sum = 0;
  if (has_top) for (int k = 0; k < size; ++k) sum += top[k];
  if (has_left) for (int k = 0; k < size; ++k) sum += d[-1 + k * kBps];
  const int shift = size == 16 ? 3 : 2;
  return has_top && has_left ? (sum + size) >> (shift + 2) : (sum + (size >> 1)) >> (shift + 1);
}

// the neighbours of macroblock (x, y) of a plane around d, by lanes [first, first + block + 1 + block (+ 4))
__device__ inline void fetch_lane(const uint8_t* plane, int stride, int x, int y, int block, int mbw, uint8_t* d, bool top_right, int k) {
  const uint8_t* at = plane + (size_t)y * block * stride + (size_t)x * block;
  if (k < block) {  // the row above
    d[-kBps + k] = y > 0 ? at[-stride + k] : 127;
  } else if (k == block) {  // the corner
    d[-kBps - 1] = y == 0 ? 127 : x > 0 ? at[-stride - 1] : 129;
  } else if (k < 2 * block + 1) {  // the column to the left
    const int r = k - block - 1;
    d[-1 + r * kBps] = x > 0 ? at[(size_t)r * stride - 1] : 129;
  } else if (top_right && k < 2 * block + 5) {
    const int c = k - 2 * block - 1;
    d[-kBps + 16 + c] = y == 0 ? 127 : x < mbw - 1 ? at[-stride + 16 + c] : at[-stride + 15];
  }
}

__global__ __launch_bounds__(kVp8Waves * 64) void vp8_recon_kernel(const Vp8ImageDesc* __restrict__ imgs) {
  __shared__ int16_t s_c[kVp8Waves][25 * 16];
  __shared__ uint8_t s_y[kVp8Waves][kYArea], s_u[kVp8Waves][kCArea], s_v[kVp8Waves][kCArea];
  const Vp8ImageDesc I = imgs[blockIdx.x];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int mw = I.mb_w, mh = I.mb_h, ys = 16 * mw, cs = 8 * mw;
  int16_t* c = s_c[wave];
  uint8_t *yd = s_y[wave] + kBps + 4, *ud = s_u[wave] + kBps + 4, *vd = s_v[wave] + kBps + 4;
  const int steps = mw + 2 * (mh - 1);
  for (int d = 0; d < steps; ++d) {
    int lo, hi;
    diagonal(d, mw, mh, lo, hi);
    for (int y0 = lo; y0 <= hi; y0 += kVp8Waves) {  // (the same trip count for every wave: the barriers below are the workgroup's)
      const int y = y0 + wave, x = d - 2 * y;
      const bool active = y <= hi;
      Mb m;
      if (active) {
        m = I.mbs[(size_t)y * mw + x];
        for (int k = lane; k < 25 * 16; k += 64) c[k] = 0;
      }
      __syncthreads();
      if (active) {
        if (lane < 25 && (m.present >> lane & 1)) {
          const int16_t* src = I.coeffs + ((size_t)m.coeff_off + __popc(m.present & ((1u << lane) - 1))) * 16;
          for (int k = 0; k < 16; ++k) c[16 * lane + k] = src[k];
        }
        fetch_lane(I.y, ys, x, y, 16, mw, yd, true, lane);
        if (lane < 32) {
          fetch_lane(I.u, cs, x, y, 8, mw, ud, false, lane);
          fetch_lane(I.v, cs, x, y, 8, mw, vd, false, lane);
        }
      }
      __syncthreads();
      if (active) {
        if (!m.is_i4x4) {  // 16x16: four pixels a lane; the Y2 block meanwhile on lane 0
          const int py = lane >> 2, px = (lane & 3) * 4;
          uint8_t out[4];
          for (int k = 0; k < 4; ++k) out[k] = (uint8_t)predict_px(m.modes[0], yd, 16, y > 0, x > 0, px + k, py);
          for (int k = 0; k < 4; ++k) yd[py * kBps + px + k] = out[k];  // (the borders read above lie outside the block)
          if (lane == 0) wht(c + 24 * 16, c);  // reads the Y2 block, writes the 16 DCs: the transforms run behind the barrier
        } else if (lane == 0) {  // B_PRED: the sub-blocks in raster order
          for (int r = 1; r < 4; ++r)
            for (int k = 0; k < 4; ++k) yd[(4 * r - 1) * kBps + 16 + k] = yd[-kBps + 16 + k];
          for (int n = 0; n < 16; ++n) {
            uint8_t* at = yd + (n >> 2) * 4 * kBps + (n & 3) * 4;
            predict4(m.modes[n], at);
            transform_class((int)(m.nz_y >> (30 - 2 * n)) & 3, c + 16 * n, at, kBps);
          }
        }
        if (lane >= 32) {  // chroma: U on lanes 32 .. 47, V on 48 .. 63, four pixels each
          const int l = lane & 15, py = l >> 1, px = (l & 1) * 4;
          uint8_t* dd = lane < 48 ? ud : vd;
          uint8_t out[4];
          for (int k = 0; k < 4; ++k) out[k] = (uint8_t)predict_px(m.uvmode, dd, 8, y > 0, x > 0, px + k, py);
          for (int k = 0; k < 4; ++k) dd[py * kBps + px + k] = out[k];
        }
      }
      __syncthreads();
      if (active) {  // the inverse transforms, a block a lane
        if (lane < 16) {
          if (!m.is_i4x4) transform_class((int)(m.nz_y >> (30 - 2 * lane)) & 3, c + 16 * lane, yd + (lane >> 2) * 4 * kBps + (lane & 3) * 4, kBps);
        } else if (lane < 24) {
          const int p = (lane - 16) >> 2, n = lane & 3;
          const uint32_t codes = (m.nz_uv >> (8 * p)) & 0xff;
          uint8_t* at = (p ? vd : ud) + (n >> 1) * 4 * kBps + (n & 1) * 4;
          const int16_t* in = c + 16 * lane;
          if (codes & 0xaa) transform_full(in, at, kBps);
          else if (in[0]) transform_dc(in, at, kBps);
        }
      }
      __syncthreads();
      if (active) {  // the macroblock -> the planes, a dword a lane
        {
          const int py = lane >> 2, px = (lane & 3) * 4;
          const uint8_t* sp = yd + py * kBps + px;
          *(uint32_t*)(I.y + ((size_t)y * 16 + py) * ys + x * 16 + px) = sp[0] | (sp[1] << 8) | (sp[2] << 16) | ((uint32_t)sp[3] << 24);
        }
        if (lane < 32) {
          const int l = lane & 15, py = l >> 1, px = (l & 1) * 4;
          const uint8_t* sp = (lane < 16 ? ud : vd) + py * kBps + px;
          uint8_t* plane = lane < 16 ? I.u : I.v;
          *(uint32_t*)(plane + ((size_t)y * 8 + py) * cs + x * 8 + px) = sp[0] | (sp[1] << 8) | (sp[2] << 16) | ((uint32_t)sp[3] << 24);
        }
      }
    }
    __threadfence_block();
    __syncthreads();  // the next diagonal reads what this one wrote
  }
}

__global__ __launch_bounds__(kVp8Waves * 64) void vp8_filter_kernel(const Vp8ImageDesc* __restrict__ imgs) {
  const Vp8ImageDesc I = imgs[blockIdx.x];
  if (!I.filter_type) return;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int mw = I.mb_w, mh = I.mb_h, ys = 16 * mw, cs = 8 * mw;
  const int steps = mw + 2 * (mh - 1);
  for (int d = 0; d < steps; ++d) {
    int lo, hi;
    diagonal(d, mw, mh, lo, hi);
    for (int y0 = lo; y0 <= hi; y0 += kVp8Waves) {
      const int y = y0 + wave, x = d - 2 * y;
      const bool active = y <= hi && lane < 32;
      Mb m;
      uint8_t* p = nullptr;  // the macroblock in this lane's plane
      int stride = 0, k = 0;
      if (active) {
        m = I.mbs[(size_t)y * mw + x];
        k = lane < 16 ? lane : lane & 7;
        stride = lane < 16 ? ys : cs;
        p = lane < 16 ? I.y + (size_t)y * 16 * ys + x * 16 : (lane < 24 ? I.u : I.v) + (size_t)y * 8 * cs + x * 8;
      }
      const bool on = active && m.level;
      if (on) filter_line(m, I.filter_type, x > 0, p + (size_t)k * stride, 1, lane >= 16);
      __threadfence_block();
      __syncthreads();
      if (on) filter_line(m, I.filter_type, y > 0, p + k, stride, lane >= 16);
    }
    __threadfence_block();
    __syncthreads();
  }
}

__global__ __launch_bounds__(kVp8Block) void vp8_convert_kernel(const Vp8ImageDesc* __restrict__ imgs) {
  const Vp8ImageDesc I = imgs[blockIdx.y];
  const int w = I.width, h = I.height, ys = 16 * I.mb_w, cs = 8 * I.mb_w, cw = (w + 1) >> 1, ch = (h + 1) >> 1;
  const long npx = (long)w * h;
  long head = (long)((uintptr_t)I.bgr & 3);
  if (head > npx) head = npx;
  for (unsigned unit = blockIdx.x * kVp8Block + threadIdx.x; unit < I.units; unit += gridDim.x * kVp8Block) {
    const long first = unit == 0 ? 0 : head + (long)(unit - 1) * kVp8Group;
    long last = unit == 0 ? head : first + kVp8Group;
    if (last > npx) last = npx;
    const int n = (int)(last - first);
    if (n <= 0) continue;
    uint8_t px[3 * kVp8Group];
    int x = (int)(first % w), y = (int)(first / w);
    for (int k = 0; k < n; ++k) {
      yuv_to_bgr(I.y[(size_t)y * ys + x], upsample(I.u, cs, x, y, w, cw, ch), upsample(I.v, cs, x, y, w, cw, ch), px + 3 * k);
      if (++x == w) { x = 0; ++y; }
    }
    uint8_t* out = I.bgr + 3 * first;
    if (n == kVp8Group && unit != 0) {
      uint32_t* o = (uint32_t*)out;
      for (int k = 0; k < 3; ++k) o[k] = px[4 * k] | (px[4 * k + 1] << 8) | (px[4 * k + 2] << 16) | ((uint32_t)px[4 * k + 3] << 24);
    } else {
      for (int k = 0; k < 3 * n; ++k) out[k] = px[k];
    }
  }
}

}  // namespace

void launch_vp8(const Vp8ImageDesc* imgs, int nimg, bool any_filter, unsigned max_units, hipStream_t s) {
  if (nimg <= 0) return;
  hipLaunchKernelGGL(vp8_recon_kernel, dim3((unsigned)nimg), dim3(kVp8Waves * 64), 0, s, imgs);
  if (any_filter) hipLaunchKernelGGL(vp8_filter_kernel, dim3((unsigned)nimg), dim3(kVp8Waves * 64), 0, s, imgs);
  unsigned gx = (max_units + kVp8Block - 1) / kVp8Block;
  if (gx > (unsigned)kVp8MaxGrid) gx = kVp8MaxGrid;
  if (gx < 1) gx = 1;
  hipLaunchKernelGGL(vp8_convert_kernel, dim3(gx, (unsigned)nimg), dim3(kVp8Block), 0, s, imgs);
}

}  // namespace ocr
