// TIFF chunk expansion on the device: one chunk per wavefront, to the bytes of tiff::expand (host/tiff_decode.h).
//
// LZW without chains.  Every table entry is a string that already stands in the chunk's output - entry `next` is the string
// of the code before plus one byte, and that is exactly what lies at the place the code before was written, one byte longer -
// so an entry is (position, length) and a code is a copy inside the chunk, made by the lanes 64 bytes at a time.  The walk
// over the codes is serial and wave-uniform: the coded bytes come through a window in LDS (filled by the lanes together, read
// through readfirstlane), so the accumulator, the width, `next` and every position stay in scalar registers and every branch
// is a scalar branch; lane 0 alone writes the table.  A copy never overlaps its source: an entry ends at or before the place
// its code is written, except the entry made by the very code that uses it (code == next: the string before plus its own first
// byte), and there the last byte is fetched from the string's first byte, which was written by an earlier code.  Loads see the
// stores of earlier codes because both are the same wavefront's vector memory operations on the same addresses, which the
// hardware keeps in order.
//
// PackBits and stored chunks have the same shape with no table: control bytes walked uniformly through the window, a literal
// run a copy from the pool, a repeat run a fill.
//
// Memory safety does not rest on the host's extent scan (tiff::coded_fault), which is what makes the result right: coded bytes
// are read below byte_len only, a table entry below `next` only (those were written since the last clear, and lie below the
// write position), and every write is cut at `need` <= nominal.  The walk ends because every step consumes coded bytes.
//
// LDS a chunk (a workgroup): LZW 16384 B positions + 8192 B lengths + 1024 B window = 25600 B, 6 chunks a CU (160 KiB);
// PackBits / stored 1024 B.
#include "kernels_tiff_lzw.h"

namespace ocr {

namespace {

__device__ inline uint32_t uni(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }

struct CodedBytes {  // a chunk's coded bytes, kTiffLzwWindow of them in LDS at a time
  const uint8_t* seg;
  uint8_t* win;
  uint32_t len, base;
  int lane;
  __device__ void stage(uint32_t from) {
    __syncthreads();
    base = from;
    for (int j = lane; j < kTiffLzwWindow; j += kTiffLzwWave) win[j] = from + (uint32_t)j < len ? seg[from + (uint32_t)j] : 0;
    __syncthreads();
  }
  __device__ uint32_t at(uint32_t i) {  // i < len, and never below an i asked before
    if (i - base >= (uint32_t)kTiffLzwWindow) stage(i);
    return uni(win[i - base]);
  }
};

// out[from .. to) = 0: bytes up to a 16-byte boundary, 16 bytes a lane, bytes again
__device__ void zero(uint8_t* out, uint32_t from, uint32_t to, int lane) {
  uint32_t head = (uint32_t)((16 - ((uintptr_t)(out + from) & 15)) & 15);
  if (head > to - from) head = to - from;
  if ((uint32_t)lane < head) out[from + (uint32_t)lane] = 0;
  from += head;
  const uint32_t quads = (to - from) / 16;
  uint4* q = reinterpret_cast<uint4*>(out + from);
  for (uint32_t k = (uint32_t)lane; k < quads; k += kTiffLzwWave) q[k] = make_uint4(0, 0, 0, 0);
  from += quads * 16;
  if ((uint32_t)lane < to - from) out[from + (uint32_t)lane] = 0;
}

// tiff::detail::unlzw, code for code; the bytes written (== need for a stream that passed lzw_extent)
__device__ uint32_t expand_lzw(CodedBytes& in, uint8_t* out, uint32_t need, uint32_t* pos, uint16_t* len) {
  const int lane = in.lane;
  uint32_t bits = 9, next = 258, acc = 0, have = 0, i = 0, o = 0;
  uint32_t old_at = 0, old_len = 0;  // where the string of the code before stands
  bool first = true;                 // the next code follows a clear
  while (o < need) {
    while (have < bits && i < in.len) { acc = (acc << 8) | in.at(i++); have += 8; }  // (at most 11 + 8 bits)
    if (have < bits) break;
    const uint32_t code = (acc >> (have - bits)) & ((1u << bits) - 1);
    have -= bits;
    if (code == 256) { bits = 9; next = 258; first = true; continue; }
    if (code == 257) break;
    if (first) {
      if (code > 255) break;
      if (lane == 0) out[o] = (uint8_t)code;
      old_at = o; old_len = 1; first = false;
      ++o;
      continue;
    }
    if (code > next || next >= (uint32_t)kTiffLzwEntries) break;
    if (lane == 0) { pos[next] = old_at; len[next] = (uint16_t)(old_len + 1); }
    ++next;
    if (next > (1u << bits) - 2 && bits < 12) ++bits;
    uint32_t l = 1;
    if (code < 256) {
      if (lane == 0) out[o] = (uint8_t)code;
    } else if (code == next - 1) {  // the string before plus its own first byte
      l = old_len + 1;
      const uint32_t take = l < need - o ? l : need - o;
      for (uint32_t k = (uint32_t)lane; k < take; k += kTiffLzwWave) out[o + k] = out[old_at + (k < old_len ? k : 0)];
    } else {
      const uint32_t from = uni(pos[code]);
      l = uni(len[code]);
      const uint32_t take = l < need - o ? l : need - o;
      for (uint32_t k = (uint32_t)lane; k < take; k += kTiffLzwWave) out[o + k] = out[from + k];
    }
    old_at = o; old_len = l;
    o += l < need - o ? l : need - o;
  }
  return o;
}

// tiff::detail::unpack_bits, control byte for control byte
__device__ uint32_t expand_packbits(CodedBytes& in, uint8_t* out, uint32_t need) {
  const uint32_t n = in.len, lane = (uint32_t)in.lane;
  uint32_t i = 0, o = 0;
  while (o < need && i < n) {
    const int c = (int8_t)in.at(i++);
    if (c >= 0) {
      uint32_t k = (uint32_t)c + 1;
      if (n - i < k) k = n - i;
      if (k > need - o) k = need - o;
      for (uint32_t j = lane; j < k; j += kTiffLzwWave) out[o + j] = in.seg[i + j];
      i += (uint32_t)c + 1; o += k;
      if (i > n) break;
    } else if (c != -128) {
      if (i >= n) break;
      const uint8_t v = (uint8_t)in.at(i++);
      uint32_t k = (uint32_t)(1 - c);
      if (k > need - o) k = need - o;
      for (uint32_t j = lane; j < k; j += kTiffLzwWave) out[o + j] = v;
      o += k;
    }
  }
  return o;
}

__global__ __launch_bounds__(kTiffLzwWave) void tiff_lzw_kernel(const TiffChunkDesc* __restrict__ chunks, const uint8_t* __restrict__ pool, uint8_t* out_all) {
  __shared__ uint32_t pos[kTiffLzwEntries];
  __shared__ uint16_t len[kTiffLzwEntries];
  __shared__ __attribute__((aligned(16))) uint8_t win[kTiffLzwWindow];
  const TiffChunkDesc k = chunks[blockIdx.x];
  CodedBytes in{pool + k.src, win, k.byte_len, 0, (int)threadIdx.x};
  uint8_t* out = out_all + k.dst;
  const uint32_t need = k.need < k.nominal ? k.need : k.nominal;
  in.stage(0);
  const uint32_t o = expand_lzw(in, out, need, pos, len);
  zero(out, o, k.nominal, in.lane);
}

__global__ __launch_bounds__(kTiffLzwWave) void tiff_runs_kernel(const TiffChunkDesc* __restrict__ chunks, const uint8_t* __restrict__ pool, uint8_t* out_all) {
  __shared__ __attribute__((aligned(16))) uint8_t win[kTiffLzwWindow];
  const TiffChunkDesc k = chunks[blockIdx.x];
  CodedBytes in{pool + k.src, win, k.byte_len, 0, (int)threadIdx.x};
  uint8_t* out = out_all + k.dst;
  const uint32_t need = k.need < k.nominal ? k.need : k.nominal;
  uint32_t o;
  if (k.compression == 1) {  // stored: a plain copy into place
    o = need < k.byte_len ? need : k.byte_len;
    for (uint32_t j = threadIdx.x; j < o; j += kTiffLzwWave) out[j] = in.seg[j];
  } else {
    in.stage(0);
    o = expand_packbits(in, out, need);
  }
  zero(out, o, k.nominal, in.lane);
}

}  // namespace

void launch_tiff_expand(const TiffChunkDesc* chunks, uint32_t lzw, uint32_t runs, const uint8_t* pool, uint8_t* out, hipStream_t s) {
  if (lzw) hipLaunchKernelGGL(tiff_lzw_kernel, dim3(lzw), dim3(kTiffLzwWave), 0, s, chunks, pool, out);
  if (runs) hipLaunchKernelGGL(tiff_runs_kernel, dim3(runs), dim3(kTiffLzwWave), 0, s, chunks + lzw, pool, out);
}

}  // namespace ocr
