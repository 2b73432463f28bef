// zlib streams inflated on the device: one stream per wavefront, to the bytes and the verdict zlib gives the host.
//
// The walk itself is inflate_core.h, which also compiles as plain C++ for one lane (host/inflate_check.cpp, run under the
// sanitizers: nobody can debug this kernel on the card).  It is serial and wave-uniform: coded bytes come through a window in
// LDS that all lanes fill, four bytes at a time into a 64-bit accumulator (LSB first) that lives with the block state and the
// output position in scalar registers (readfirstlane), so every branch of the walk is a scalar branch.  A symbol is one lookup
// in an LDS table - the next 10 bits for a literal/length code, 8 for a distance code, and a second level for longer codes -
// never a walk bit by bit; the fixed code's tables are built by the same routine and kept while fixed blocks follow each
// other.  The lanes work together on the window, the table build (counts, one lane per code length for the codes, one lane
// per slot for the second level's room), the stored blocks and the matches, 64 bytes a step.  Literals are collected in an LDS
// line of 256 bytes and stored by the lanes when it is full and before anything that may read them (a match, a stored block,
// the end).  Only the code-length alphabet (HCLEN, 16 / 17 / 18) is decoded serially by nature.
//
// A match copies out[o + k] = out[o - distance + k % distance]: its sources lie strictly below `o`, and were stored by earlier
// vector stores of this wavefront (the line is stored before the match), which later loads of the same wavefront on the same
// addresses see - the ordering argument of kernels_tiff_lzw.hip.  A distance above `o` is a fault; the window is 32 KiB
// whatever the header's CINFO says, as in zlib.
//
// Memory safety rests on nothing outside this file and inflate_core.h - no host scan stands in front of the launch: coded
// bytes are read below byte_len only, table indices are masked or checked against the table, every write is cut at
// min(need, nominal).  Every step of the walk consumes at least one bit or ends it, and a bit beyond the stream's end ends it.
//
// LDS a stream (a workgroup): 2048 B window + 256 B line + 5120 B literal/length table + 1536 B distance table + 352 B code
// lengths + 4240 B for the table build = 13552 B: 160 KiB / 13552 B = 12 streams a CU by LDS; the walk is latency-bound and lives on that.
#define INFLATE_CORE_DEVICE 1
#include "kernels_inflate.h"

#include "inflate_core.h"

namespace ocr {

namespace {

static_assert(sizeof(inflate_core::Shared) <= 40 * 1024, "at least four streams a CU");

// out[from .. to) = 0: bytes up to a 16-byte boundary, 16 bytes a lane, bytes again
__device__ void zero(uint8_t* out, uint32_t from, uint32_t to, uint32_t lane) {
  uint32_t head = (uint32_t)((16 - ((uintptr_t)(out + from) & 15)) & 15);
  if (head > to - from) head = to - from;
  if (lane < head) out[from + lane] = 0;
  from += head;
  const uint32_t quads = (to - from) / 16;
  uint4* q = reinterpret_cast<uint4*>(out + from);
  for (uint32_t k = lane; k < quads; k += kInflateWave) q[k] = make_uint4(0, 0, 0, 0);
  from += quads * 16;
  if (lane < to - from) out[from + lane] = 0;
}

__global__ __launch_bounds__(kInflateWave) void inflate_kernel(const InflateDesc* __restrict__ streams, const uint8_t* __restrict__ pool, uint8_t* out_all,
                                                                uint32_t* __restrict__ produced) {
  __shared__ inflate_core::Shared sh;
  const InflateDesc k = streams[blockIdx.x];
  const uint32_t need = k.need < k.nominal ? k.need : k.nominal;
  uint8_t* out = out_all + k.dst;
  inflate_core::Walk walk(sh, inflate_core::Stream{pool + k.src, k.byte_len, out, need});
  const uint32_t o = walk.run();
  zero(out, o, k.nominal, threadIdx.x);
  if (threadIdx.x == 0) produced[blockIdx.x] = o;
}

}  // namespace

void launch_inflate(const InflateDesc* streams, uint32_t count, const uint8_t* pool, uint8_t* out, uint32_t* produced, hipStream_t s) {
  if (count) hipLaunchKernelGGL(inflate_kernel, dim3(count), dim3(kInflateWave), 0, s, streams, pool, out, produced);
}

}  // namespace ocr
