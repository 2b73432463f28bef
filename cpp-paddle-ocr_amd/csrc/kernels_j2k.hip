// The sample half of the JPEG 2000 decoder on the device (kernels_j2k.h): per level one horizontal and one vertical launch
// over every image, tile and component of a batch that has the level, and one finishing launch.
//
// A workgroup lifts a window of a row or column in LDS.  A window carries kJ2kHalo samples either side of what it writes: a
// lifting step reaches one sample, the 9/7 has four of them, so the samples a window writes depend on nothing outside it, and
// the halo is computed again by the neighbouring window with the same operations on the same values - the bytes do not depend
// on where the windows fall.  At a band's edge the missing neighbour is the one on the other side (a select, no branch); a
// neighbour outside the window is clamped into it and only ever feeds halo samples.
//   rows:    256 threads take 4 rows x 256 samples; lane t reads sample t of the window - even coordinates from the low-pass
//            half of the row, odd ones from the high-pass half, two contiguous streams - and dequantises a band on this first
//            read (the low-pass quadrant of a level above the first comes reconstructed from plane r).  Written to plane b.
//   columns: 256 threads take 64 columns x 64 rows; a wave reads 64 contiguous samples of a row, so the vertical pass reads
//            HBM row by row, and lifts along LDS columns (bank = lane, no conflict).  Written to plane r.
//   finish:  the columns of the last level for the (1 or 3) components of a tile at once, then j2k::finish - component transform,
//            rounding, level shift, clamp, precision reduction - straight into the packed BGR image.
// The file is compiled without contraction (build.py), so x + (l + r) * c is two roundings, as in j2k_decode.h on the host.
#include "kernels_j2k.h"

namespace ocr {

using PaddleOCR::j2k::Rect;
namespace j2k = PaddleOCR::j2k;

namespace {

__device__ inline int clampi(int v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : v; }

__global__ __launch_bounds__(kJ2kBlock) void j2k_rows_kernel(J2kBatch B, uint32_t first) {
  __shared__ int32_t win[kJ2kRows][kJ2kRowWin];
  const J2kUnit u = B.units[first + blockIdx.x];
  const J2kTc tc = B.tcs[u.job];
  const Rect full{tc.x0, tc.y0, tc.x1, tc.y1};
  const int lev = tc.levels - u.r;
  const Rect cur = j2k::res_rect(full, lev), low = j2k::res_rect(full, lev + 1);
  const int cw = cur.x1 - cur.x0, ch = cur.y1 - cur.y0, lw = low.x1 - low.x0, lh = low.y1 - low.y0, w = tc.x1 - tc.x0;
  const int t = threadIdx.x, p = u.p - kJ2kHalo + t;
  const bool inside = p >= 0 && p < cw;
  const int ux = cur.x0 + p;
  const bool odd = ux & 1;
  const int sx = odd ? lw + ((ux >> 1) - (cur.x0 >> 1)) : (ux >> 1) - low.x0;
  const float* steps = B.steps + tc.step_off;
#pragma unroll
  for (int k = 0; k < kJ2kRows; ++k) {
    const int y = u.q + k;
    int32_t v = 0;
    if (inside && y < ch) {
      const size_t at = (size_t)tc.plane + (size_t)y * w + sx;
      if (!odd && y < lh) v = u.r > 1 ? B.r[at] : j2k::dequant(B.a[at], tc.transform, steps[0]);
      else v = j2k::dequant(B.a[at], tc.transform, steps[3 * (u.r - 1) + (odd ? 1 : 0) + (y >= lh ? 2 : 0)]);
    }
    win[k][t] = v;
  }
  __syncthreads();
  const int base = u.p - kJ2kHalo;
  const int tl = clampi((p > 0 ? p - 1 : p + 1) - base, 0, kJ2kRowWin - 1), tr = clampi((p + 1 < cw ? p + 1 : p - 1) - base, 0, kJ2kRowWin - 1);
  if (cw == 1) {
    if (!tc.transform && odd && inside)
      for (int k = 0; k < kJ2kRows; ++k) win[k][t] = j2k::half_trunc(win[k][t]);
  } else if (!tc.transform) {
    if (!odd && inside)
      for (int k = 0; k < kJ2kRows; ++k) win[k][t] = j2k::lift53_even(win[k][t], win[k][tl], win[k][tr]);
    __syncthreads();
    if (odd && inside)
      for (int k = 0; k < kJ2kRows; ++k) win[k][t] = j2k::lift53_odd(win[k][t], win[k][tl], win[k][tr]);
  } else {
    float(*f)[kJ2kRowWin] = reinterpret_cast<float(*)[kJ2kRowWin]>(win);
    for (int k = 0; k < kJ2kRows; ++k) f[k][t] = f[k][t] * (odd ? j2k::kTwoInvK : j2k::kK);
    const float c[4] = {-j2k::kDelta, -j2k::kGamma, -j2k::kBeta, -j2k::kAlpha};
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      __syncthreads();
      if (odd == (bool)(s & 1) && inside)
        for (int k = 0; k < kJ2kRows; ++k) f[k][t] = j2k::lift97(f[k][t], f[k][tl], f[k][tr], c[s]);
    }
  }
  // (every lane writes only what it computed itself: no barrier needed before the store)
  if (inside && t >= kJ2kHalo && t < kJ2kRowWin - kJ2kHalo)
    for (int k = 0; k < kJ2kRows; ++k)
      if (u.q + k < ch) B.b[(size_t)tc.plane + (size_t)(u.q + k) * w + p] = win[k][t];
}

// the window of rows [a - halo, a - halo + kJ2kColWin) of columns [x0, x0 + 64) of resolution r of a tile-component, lifted
// along the columns; r == 0 (a component without a transform): the dequantised samples
__device__ void cols_window(const J2kBatch& B, const J2kTc& tc, int r, int x0, int a, int32_t (*win)[kJ2kCols]) {
  const Rect full{tc.x0, tc.y0, tc.x1, tc.y1};
  const int lev = tc.levels - r;
  const Rect cur = j2k::res_rect(full, lev), low = j2k::res_rect(full, lev + 1);
  const int cw = cur.x1 - cur.x0, ch = cur.y1 - cur.y0, lh = low.y1 - low.y0, w = tc.x1 - tc.x0;
  const int lane = threadIdx.x & 63, g = threadIdx.x >> 6, x = x0 + lane, base = a - kJ2kHalo;
  for (int k = g; k < kJ2kColWin; k += kJ2kBlock / 64) {
    const int i = base + k;
    int32_t v = 0;
    if (i >= 0 && i < ch && x < cw) {
      if (r == 0) {
        v = j2k::dequant(B.a[(size_t)tc.plane + (size_t)i * w + x], tc.transform, B.steps[tc.step_off]);
      } else {
        const int uy = cur.y0 + i;
        const int sy = (uy & 1) ? lh + ((uy >> 1) - (cur.y0 >> 1)) : (uy >> 1) - low.y0;
        v = B.b[(size_t)tc.plane + (size_t)sy * w + x];
      }
    }
    win[k][lane] = v;
  }
  __syncthreads();
  if (r == 0) return;
  if (ch == 1) {
    if (!tc.transform && (cur.y0 & 1) && g == 0 && base + kJ2kHalo == 0) win[kJ2kHalo][lane] = j2k::half_trunc(win[kJ2kHalo][lane]);
    __syncthreads();
    return;
  }
  float(*f)[kJ2kCols] = reinterpret_cast<float(*)[kJ2kCols]>(win);
  const float c[4] = {-j2k::kDelta, -j2k::kGamma, -j2k::kBeta, -j2k::kAlpha};
  const int nsteps = tc.transform ? 5 : 2;
  for (int s = 0; s < nsteps; ++s) {
    for (int k = g; k < kJ2kColWin; k += kJ2kBlock / 64) {
      const int i = base + k;
      if (i < 0 || i >= ch) continue;
      const bool odd = (cur.y0 + i) & 1;
      const int kl = clampi((i > 0 ? i - 1 : i + 1) - base, 0, kJ2kColWin - 1), kr = clampi((i + 1 < ch ? i + 1 : i - 1) - base, 0, kJ2kColWin - 1);
      if (!tc.transform) {
        if (s == 0 && !odd) win[k][lane] = j2k::lift53_even(win[k][lane], win[kl][lane], win[kr][lane]);
        if (s == 1 && odd) win[k][lane] = j2k::lift53_odd(win[k][lane], win[kl][lane], win[kr][lane]);
      } else if (s == 0) {
        f[k][lane] = f[k][lane] * (odd ? j2k::kTwoInvK : j2k::kK);
      } else if (odd == (bool)((s - 1) & 1)) {
        f[k][lane] = j2k::lift97(f[k][lane], f[kl][lane], f[kr][lane], c[s - 1]);
      }
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(kJ2kBlock) void j2k_cols_kernel(J2kBatch B, uint32_t first) {
  __shared__ int32_t win[kJ2kColWin][kJ2kCols];
  const J2kUnit u = B.units[first + blockIdx.x];
  const J2kTc tc = B.tcs[u.job];
  cols_window(B, tc, u.r, u.p, u.q, win);
  const Rect cur = j2k::res_rect(Rect{tc.x0, tc.y0, tc.x1, tc.y1}, tc.levels - u.r);
  const int cw = cur.x1 - cur.x0, ch = cur.y1 - cur.y0, w = tc.x1 - tc.x0;
  const int lane = threadIdx.x & 63, g = threadIdx.x >> 6, x = u.p + lane;
  for (int k = kJ2kHalo + g; k < kJ2kColWin - kJ2kHalo; k += kJ2kBlock / 64) {
    const int i = u.q - kJ2kHalo + k;
    if (i < ch && x < cw) B.r[(size_t)tc.plane + (size_t)i * w + x] = win[k][lane];
  }
}

__global__ __launch_bounds__(kJ2kBlock) void j2k_finish_kernel(J2kBatch B, uint32_t first) {
  __shared__ int32_t win[3][kJ2kColWin][kJ2kCols];
  const J2kUnit u = B.units[first + blockIdx.x];
  const J2kTile tile = B.tiles[u.job];
  const J2kTc tc0 = B.tcs[tile.tc[0]];
  for (int c = 0; c < tile.ncomp; ++c) cols_window(B, B.tcs[tile.tc[c]], tc0.levels, u.p, u.q, win[c]);
  const int w = tc0.x1 - tc0.x0, h = tc0.y1 - tc0.y0;
  const int lane = threadIdx.x & 63, g = threadIdx.x >> 6, x = u.p + lane;
  for (int k = kJ2kHalo + g; k < kJ2kColWin - kJ2kHalo; k += kJ2kBlock / 64) {
    const int i = u.q - kJ2kHalo + k;
    if (i >= h || x >= w) continue;
    const int32_t s[3] = {win[0][k][lane], tile.ncomp > 1 ? win[1][k][lane] : 0, tile.ncomp > 1 ? win[2][k][lane] : 0};
    uint8_t px[3];
    j2k::finish(s, tile.ncomp, tile.transform, tile.mct, tile.prec, tile.chan, px);
    uint8_t* out = tile.dst + ((size_t)(tile.oy + i) * tile.img_w + (size_t)(tile.ox + x)) * 3;
    out[0] = px[0]; out[1] = px[1]; out[2] = px[2];
  }
}

}  // namespace

void launch_j2k(const J2kBatch& batch, const J2kStep* steps, int nsteps, uint32_t fin_first, uint32_t fin_count, hipStream_t s) {
  for (int i = 0; i < nsteps; ++i) {
    if (steps[i].h_count) hipLaunchKernelGGL(j2k_rows_kernel, dim3(steps[i].h_count), dim3(kJ2kBlock), 0, s, batch, steps[i].h_first);
    if (steps[i].v_count) hipLaunchKernelGGL(j2k_cols_kernel, dim3(steps[i].v_count), dim3(kJ2kBlock), 0, s, batch, steps[i].v_first);
  }
  if (fin_count) hipLaunchKernelGGL(j2k_finish_kernel, dim3(fin_count), dim3(kJ2kBlock), 0, s, batch, fin_first);
}

}  // namespace ocr
