// CCITT fax expansion on the device: one chunk per wavefront, to the bytes of tiff::unfax_all (host/ccitt_decode.h, whose
// walk() this follows code for code; the tables are that header's, built at compile time into global memory).
//
// The walk over the codes is serial and wave-uniform: the coded bytes come through a window in LDS (filled by the lanes
// together, read through readfirstlane), the tables are read with wave-uniform indices, so the bit position, a0, the colour and
// the reference row's cursor stay in scalar registers and every branch of the walk is a scalar branch - but for one: a row is
// kept as the list of its changing elements, not as bits (two lists in LDS, the row being coded and its reference row, swapped
// per row), and the append is a store under `lane == 0`, the walk's one divergent instruction.  The lanes' share is turning
// a finished list into the row's bytes: a lane takes a 32-bit word of the row (or a byte, where the row is not aligned), finds
// the colour at its first pixel by a binary search in the list and walks the changes inside it.  Stores are plain vector
// stores.
//
// Memory safety does not rest on the host's scan (tiff::fax_fault_of), which is what makes the result right: coded bytes are
// read below byte_len only (the window holds zeros behind them), an append is checked against width + 1 <= the list's room,
// the reference list is read below its count only, a row is written only where it lies wholly below the chunk's nominal size,
// and a width beyond kTiffFaxMaxWidth writes zeros alone.  The walk ends because every step consumes at least one coded bit.
// A stream the walk cannot follow (none that passed the scan) leaves zeros from its row on.
//
// LDS a chunk (a workgroup): 2 lists x 8194 entries x 2 B = 32776 B + 1024 B window = 33800 B; by that size 4 chunks
// fit a CU's 160 KiB (derived, not measured).  The widest chunk the device route takes follows from that: kTiffFaxMaxWidth = 8192 pixels (A3 at 600 dpi is 7016 across), a
// position fits 16 bits; wider chunks go the host route.
#include "../host/ccitt_decode.h"
#include "kernels_tiff_fax.h"

namespace ocr {

namespace {

namespace ccitt = PaddleOCR::ccitt;

__device__ const ccitt::RunTable d_white = ccitt::make_runs(false);
__device__ const ccitt::RunTable d_black = ccitt::make_runs(true);
__device__ const ccitt::ModeTable d_modes = ccitt::make_modes();

__device__ inline uint32_t uni(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }

struct FaxBits {  // a chunk's coded bits, kTiffFaxWindow bytes of them in LDS at a time; behind the stream's end they read as zeros
  const uint8_t* seg;
  uint8_t* win;
  uint32_t len, base;
  int lane;
  uint64_t at;  // in bits
  __device__ void stage(uint32_t from) {
    __syncthreads();
    base = from;
    for (int j = lane; j < kTiffFaxWindow; j += kTiffFaxWave) win[j] = (uint64_t)from + (uint32_t)j < len ? seg[(uint64_t)from + (uint32_t)j] : 0;
    __syncthreads();
  }
  __device__ uint64_t left() const { return at < 8ull * len ? 8ull * len - at : 0; }
  __device__ uint32_t peek(int k) {  // the next k <= 16 bits
    const uint32_t i = (uint32_t)(at >> 3) < len ? (uint32_t)(at >> 3) : len;  // (at or behind the end: zeros)
    if (i - base > (uint32_t)(kTiffFaxWindow - 4)) stage(i);
    const uint8_t* p = win + (i - base);
    const uint32_t w = uni(((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3]);
    return (uint32_t)(w << (uint32_t)(at & 7)) >> (32 - k);
  }
};

struct FaxRow {  // the list of the row being coded
  uint16_t* cur;
  uint32_t cnt, width;
  int lane;
  __device__ bool append(uint32_t x) {
    if (cnt > width || cnt >= (uint32_t)kTiffFaxList) return false;
    if (lane == 0) cur[cnt] = (uint16_t)x;
    ++cnt;
    return true;
  }
};

// ccitt::detail::run: make-ups, then a terminating code; false where the host's walk refuses
__device__ bool fax_run(FaxBits& b, bool black, uint32_t room, uint32_t& total) {
  const ccitt::RunTable& t = black ? d_black : d_white;
  total = 0;
  for (;;) {
    const uint32_t e = uni(t.e[b.peek(ccitt::kRunBits)]), len = e >> 12, r = e & 0xFFF;
    if (!len || len > b.left()) return false;
    b.at += len;
    total += r;
    if (total > room) return false;
    if (r < 64) return true;
  }
}

// one row of ccitt::walk: the list of `row` from the stream, against ref[0 .. nr)
__device__ bool fax_row(FaxBits& b, FaxRow& row, const uint16_t* ref, uint32_t nref, uint32_t compression, uint32_t t4) {
  const uint32_t width = row.width;
  bool two_d = compression == 4;
  if (compression == 2) b.at = (b.at + 7) & ~7ull;
  else if (compression == 32771) b.at = (b.at + 15) & ~15ull;
  else if (compression == 3) {
    uint32_t zeros = 0;
    for (;;) {  // the EOL: zeros, 16 at a time, up to a 1
      if (!b.left()) return false;
      const uint32_t w = b.peek(16);
      if (w) { const uint32_t lead = (uint32_t)__builtin_clz(w) - 16; zeros += lead; b.at += lead; break; }
      zeros += 16; b.at += 16;
    }
    if (!b.left() || zeros < (uint32_t)ccitt::kEolZeros) return false;
    ++b.at;
    if (t4 & 1) {
      if (!b.left()) return false;
      two_d = !b.peek(1);
      ++b.at;
    }
  }
  if (!two_d) {
    uint32_t x = 0, r;
    bool black = false;
    while (x < width) {
      if (!fax_run(b, black, width - x, r)) return false;
      x += r;
      if (!row.append(x)) return false;
      black = !black;
    }
    return true;
  }
  int a0 = -1, bi = 0;
  const int nr = (int)nref, w = (int)width;
  bool black = false;
  while (a0 < w) {
    const uint32_t e = uni(d_modes.e[b.peek(ccitt::kModeBits)]), len = e >> 4, mode = e & 15;
    if (!len || len > b.left() || mode == ccitt::kExtension) return false;
    b.at += len;
    const int from = a0 < 0 ? 0 : a0;
    const int b1 = bi < nr ? (int)uni(ref[bi]) : w;
    if (mode == ccitt::kPass) {
      a0 = bi + 1 < nr ? (int)uni(ref[bi + 1]) : w;
      bi += 2;
    } else if (mode == ccitt::kHorizontal) {
      uint32_t r1, r2;
      if (!fax_run(b, black, (uint32_t)(w - from), r1) || !row.append((uint32_t)from + r1)) return false;
      if (!fax_run(b, !black, (uint32_t)(w - from) - r1, r2) || !row.append((uint32_t)from + r1 + r2)) return false;
      a0 = from + (int)(r1 + r2);
    } else {
      const int d = mode == ccitt::kV0 ? 0 : mode <= ccitt::kVR3 ? (int)mode - ccitt::kV0 : -((int)mode - ccitt::kVR3);
      const int a1 = b1 + d;
      if (a1 > w || a1 < from || !row.append((uint32_t)a1)) return false;
      a0 = a1;
      black = !black;
      bi += d >= 0 ? 1 : -1;
    }
    while (bi < nr && (bi < 0 || (int)uni(ref[bi]) <= a0)) bi += 2;
  }
  return true;
}

// pixels [x0, x0 + 32) of a row as a word, the first pixel in the most significant bit; pixels at and behind `width` are 0
__device__ uint32_t fax_word(const uint16_t* list, uint32_t cnt, uint32_t width, uint32_t x0) {
  uint32_t lo = 0, hi = cnt;  // the entries <= x0: their number says the colour at x0
  while (lo < hi) {
    const uint32_t mid = (lo + hi) / 2;
    if (list[mid] <= x0) lo = mid + 1;
    else hi = mid;
  }
  uint32_t idx = lo, pos = x0, word = 0;
  const uint32_t end = x0 + 32 < width ? x0 + 32 : width;
  while (pos < end) {
    const uint32_t change = idx < cnt ? list[idx] : end;  // (not below pos: the list does not decrease)
    const uint32_t next = change < end ? change : end;
    if ((idx & 1) && next > pos) {  // an odd number of changes lies at or before pos: black up to the next one
      const uint32_t r0 = pos - x0, r1 = next - x0;
      word |= (0xFFFFFFFFu >> r0) & ~(r1 < 32 ? 0xFFFFFFFFu >> r1 : 0u);
    }
    pos = next;
    ++idx;
  }
  return word;
}

// a finished list to the row's bytes: bytes up to a 4-byte boundary, words, bytes again
__device__ void fax_render(const uint16_t* list, uint32_t cnt, uint32_t width, uint8_t* row, uint32_t row_bytes, int lane) {
  uint32_t head = (uint32_t)((4 - ((uintptr_t)row & 3)) & 3);
  if (head > row_bytes) head = row_bytes;
  if ((uint32_t)lane < head) row[lane] = (uint8_t)(fax_word(list, cnt, width, 8 * (uint32_t)lane) >> 24);
  const uint32_t words = (row_bytes - head) / 4;
  uint32_t* q = reinterpret_cast<uint32_t*>(row + head);
  for (uint32_t k = (uint32_t)lane; k < words; k += kTiffFaxWave) q[k] = __builtin_bswap32(fax_word(list, cnt, width, 8 * (head + 4 * k)));
  const uint32_t tail = head + 4 * words;
  if ((uint32_t)lane < row_bytes - tail) row[tail + (uint32_t)lane] = (uint8_t)(fax_word(list, cnt, width, 8 * (tail + (uint32_t)lane)) >> 24);
}

// out[from .. to) = 0: bytes up to a 16-byte boundary, 16 bytes a lane, bytes again
__device__ void fax_zero(uint8_t* out, uint32_t from, uint32_t to, int lane) {
  uint32_t head = (uint32_t)((16 - ((uintptr_t)(out + from) & 15)) & 15);
  if (head > to - from) head = to - from;
  if ((uint32_t)lane < head) out[from + (uint32_t)lane] = 0;
  from += head;
  const uint32_t quads = (to - from) / 16;
  uint4* q = reinterpret_cast<uint4*>(out + from);
  for (uint32_t k = (uint32_t)lane; k < quads; k += kTiffFaxWave) q[k] = make_uint4(0, 0, 0, 0);
  from += quads * 16;
  if ((uint32_t)lane < to - from) out[from + (uint32_t)lane] = 0;
}

__global__ __launch_bounds__(kTiffFaxWave) void tiff_fax_kernel(const TiffFaxDesc* __restrict__ chunks, const uint8_t* __restrict__ pool, uint8_t* out_all) {
  __shared__ uint16_t lists[2][kTiffFaxList];
  __shared__ __attribute__((aligned(16))) uint8_t win[kTiffFaxWindow];
  const TiffFaxDesc k = chunks[blockIdx.x];
  const int lane = (int)threadIdx.x;
  uint8_t* out = out_all + k.dst;
  const bool fits = k.width >= 1 && k.width <= (uint32_t)kTiffFaxMaxWidth;
  const uint32_t row_bytes = fits ? (k.width + 7) / 8 : 1;
  uint32_t rows = fits ? k.rows : 0;
  if (rows > k.nominal / row_bytes) rows = k.nominal / row_bytes;  // a row is written only where it lies below `nominal`
  FaxBits b{pool + k.src, win, k.byte_len, 0, lane, 0};
  b.stage(0);
  uint32_t done = 0, nref = 0;
  for (uint32_t y = 0; y < rows; ++y) {
    FaxRow row{lists[y & 1], 0, k.width, lane};
    if (!fax_row(b, row, lists[(y & 1) ^ 1], nref, k.compression, k.t4_options)) break;
    __syncthreads();  // lane 0's appends, before the lanes read them
    fax_render(row.cur, row.cnt, k.width, out + (size_t)y * row_bytes, row_bytes, lane);
    __syncthreads();  // the list of the row before is free to be written again
    nref = row.cnt;
    done = y + 1;
  }
  fax_zero(out, done * row_bytes, k.nominal, lane);
}

}  // namespace

void launch_tiff_fax(const TiffFaxDesc* chunks, uint32_t count, const uint8_t* pool, uint8_t* out, hipStream_t s) {
  if (count) hipLaunchKernelGGL(tiff_fax_kernel, dim3(count), dim3(kTiffFaxWave), 0, s, chunks, pool, out);
}

}  // namespace ocr
