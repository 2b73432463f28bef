// JPEG 2000 tier-1 on the device: one code block per wavefront, its state in LDS.
//
// The arithmetic is j2k::t1::decode of host/j2k_decode.h - the MQ decoder, the context rules and the pass walk are that
// text, compiled here over the storage below.  The decoder is serial: every lane of the wavefront runs the same walk over the
// same values (each LDS read goes through readfirstlane, so a, c, ct, the position and every context stay in scalar registers
// and every branch is a scalar branch), lane 0 alone stores.  What is parallel the lanes share: clearing the state, staging the
// segment, clearing VISITED after a cleanup pass, and the final store to the plane, coalesced along rows.
//
// LDS a block (a workgroup): 16384 B magnitudes + 6160 B flags (a byte a sample, a border of one sample) + 256 B of the
// segment + 32 B of contexts = 22832 B, so 7 blocks a CU (160 KiB).
#include "kernels_j2k_t1.h"

namespace ocr {

namespace {

namespace j2k = PaddleOCR::j2k;

__device__ inline int uni(int v) { return __builtin_amdgcn_readfirstlane(v); }

struct LdsBlock {
  uint32_t* mg;   // w * h
  uint8_t* fl;    // (w + 2) * (h + 2), row stride fw
  uint8_t* ctx;   // 19 contexts
  uint8_t* win;   // bytes base .. base + kJ2kT1Window of the segment
  const uint8_t* seg;
  uint32_t len, base;
  int w, h, fw, lane;

  __device__ int width() const { return w; }
  __device__ int height() const { return h; }
  __device__ int flag(int x, int y) const { return uni(fl[(y + 1) * fw + x + 1]); }
  __device__ void set_flag(int x, int y, int v) { if (lane == 0) fl[(y + 1) * fw + x + 1] = (uint8_t)v; }
  __device__ uint32_t mag(int x, int y) const { return (uint32_t)uni((int)mg[y * w + x]); }
  __device__ void set_mag(int x, int y, uint32_t m) { if (lane == 0) mg[y * w + x] = m; }
  __device__ int cx(int i) const { return uni(ctx[i]); }
  __device__ void set_cx(int i, int v) { if (lane == 0) ctx[i] = (uint8_t)v; }
  // The Mq::at rule: a byte at or beyond the segment's end reads ff, so no read leaves [seg, seg + len).
  __device__ void stage(uint32_t from) {
    __syncthreads();
    base = from;
    for (int j = lane; j < kJ2kT1Window; j += kJ2kT1Wave) win[j] = from + (uint32_t)j < len ? seg[from + (uint32_t)j] : 0xff;
    __syncthreads();
  }
  __device__ int at(uint32_t i) {
    if (i >= len) return 0xff;
    if (i - base >= (uint32_t)kJ2kT1Window) stage(i ? i - 1 : 0);  // (the decoder looks one byte ahead and may step back to it)
    return uni(win[i - base]);
  }
  __device__ void clear() {
    uint32_t* f4 = reinterpret_cast<uint32_t*>(fl);
    for (int j = lane; j < (fw * (h + 2) + 3) / 4; j += kJ2kT1Wave) f4[j] = 0;
    for (int j = lane; j < w * h; j += kJ2kT1Wave) mg[j] = 0;
    stage(0);
  }
  __device__ void clear_visited() {
    __syncthreads();
    uint32_t* f4 = reinterpret_cast<uint32_t*>(fl);
    for (int j = lane; j < (fw * (h + 2) + 3) / 4; j += kJ2kT1Wave) f4[j] &= ~(0x01010101u * (uint32_t)j2k::kVisited);
    __syncthreads();
  }
};

// Termination: t1::decode runs at most `passes` <= 88 passes of w * h <= 4096 samples, each a bounded number of decoded
// symbols, each symbol at most 15 renormalisation shifts; the bytes decide values only.  Bounds: the block's fields passed
// j2k::coded_fault on the host - its rectangle lies inside its plane, its bytes inside the pool.
__global__ __launch_bounds__(kJ2kT1Wave) void j2k_t1_kernel(const J2kT1Block* __restrict__ blocks, const uint8_t* __restrict__ pool, int32_t* __restrict__ plane) {
  __shared__ uint32_t mg[kJ2kT1Samples];
  __shared__ __attribute__((aligned(16))) uint8_t fl[kJ2kT1FlagBytes];
  __shared__ __attribute__((aligned(16))) uint8_t win[kJ2kT1Window];
  __shared__ uint8_t ctx[32];
  const J2kT1Block k = blocks[blockIdx.x];
  LdsBlock s;
  s.mg = mg; s.fl = fl; s.ctx = ctx; s.win = win;
  s.seg = pool + k.byte_off;
  s.len = k.byte_len; s.base = 0;
  s.w = k.w; s.h = k.h; s.fw = k.w + 2;
  s.lane = (int)threadIdx.x;
  j2k::t1::decode(s, k.numbps, k.passes, k.orient);
  __syncthreads();
  const int n = s.w * s.h;
  for (int j = s.lane; j < n; j += kJ2kT1Wave) {
    const int y = j / s.w, x = j - y * s.w;
    plane[(size_t)k.plane + (size_t)y * k.stride + (size_t)x] = j2k::t1::coefficient(fl[(y + 1) * s.fw + x + 1], mg[j]);
  }
}

}  // namespace

void launch_j2k_t1(const J2kT1Block* blocks, uint32_t count, const uint8_t* pool, int32_t* plane, hipStream_t s) {
  if (count) hipLaunchKernelGGL(j2k_t1_kernel, dim3(count), dim3(kJ2kT1Wave), 0, s, blocks, pool, plane);
}

}  // namespace ocr
