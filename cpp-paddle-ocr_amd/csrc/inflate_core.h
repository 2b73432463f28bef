// The walk of one zlib stream (RFC 1950 / 1951), written once for two compilers: as device code for a wavefront of 64 lanes
// (kernels_inflate.hip defines INFLATE_CORE_DEVICE before it includes this file) and as plain C++ for a "wavefront" of one lane
// (host/inflate_check.cpp), where the LDS arrays are plain arrays, a barrier is nothing and readfirstlane is the identity.  The
// second form is what runs under the sanitizers; it executes the same statements with the same indices.
//
// The verdict is that of zlib 1.2.11 driven as tiff::detail::inflate drives it (host/tiff_decode.h): `produced` is the count
// of bytes that come out before the first fault, the end of the final block or the end of the input, cut at `need`.  The
// checksum behind the final block is not read.  A fault is: a bad zlib header (CM != 8, CINFO > 7, FCHECK, FDICT), block type
// 3, stored LEN != ~NLEN, HLIT > 286 or HDIST > 30, a code-length set that is over-subscribed or incomplete, a 16 with no
// length before it, a repeat past HLIT + HDIST, no end-of-block code, a literal/length or distance set that is
// over-subscribed, or incomplete unless it is a single code of one bit (zlib's exception; no code at all is let through as
// well and every symbol read from such a set is a fault), symbols 286 / 287 and distance symbols 30 / 31, a distance beyond
// the bytes written, and a symbol or field whose bits are not all inside the stream's bytes (a stored block gives the bytes
// the input has before it faults, as zlib does).
//
// Nothing here depends on what the bytes are: coded bytes are read below byte_len only (the window holds zeros behind them),
// a table index is masked to the table or checked against its allocation, and every write is cut at `need`.
#pragma once
#include <stdint.h>

#ifdef INFLATE_CORE_DEVICE
#define INFLATE_FN __device__ inline
#else
#define INFLATE_FN inline
#endif

namespace ocr {
namespace inflate_core {

#ifdef INFLATE_CORE_DEVICE
constexpr uint32_t kLanes = 64;
INFLATE_FN uint32_t lane_id() { return threadIdx.x; }
INFLATE_FN uint32_t uni(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
INFLATE_FN void sync() { __syncthreads(); }
INFLATE_FN uint32_t add(uint32_t* p, uint32_t v) { return atomicAdd(p, v); }
INFLATE_FN void raise(uint32_t* p, uint32_t v) { atomicMax(p, v); }
#else
constexpr uint32_t kLanes = 1;
INFLATE_FN uint32_t lane_id() { return 0; }
INFLATE_FN uint32_t uni(uint32_t v) { return v; }
INFLATE_FN void sync() {}
INFLATE_FN uint32_t add(uint32_t* p, uint32_t v) { const uint32_t was = *p; *p = was + v; return was; }
INFLATE_FN void raise(uint32_t* p, uint32_t v) { if (*p < v) *p = v; }
#endif

constexpr uint32_t kWindow = 2048;    // coded bytes in LDS at a time (a multiple of 4)
constexpr uint32_t kLine = 256;       // literals collected before the lanes store them
constexpr uint32_t kLitRoot = 10, kLitSub = 1536;  // literal/length: 2^10 primary entries, then the second level
constexpr uint32_t kDistRoot = 8, kDistSub = 512;  // distance
constexpr uint32_t kLitTable = (1u << kLitRoot) + kLitSub, kDistTable = (1u << kDistRoot) + kDistSub;
constexpr uint32_t kMaxSymbols = 288 + 32;
// Second level, sized per primary slot by the longest code under it: a slot whose longest code has d bits beyond the root
// holds at least d + 1 codes (a complete subtree that deep) and takes 2^d entries, so the whole level takes at most
// symbols * max(2^d / (d + 1)): 286 * 32 / 6 < 1536 and 30 * 128 / 8 < 512.  The allocation checks it all the same.

// A table entry (16 bits): 0 = no code here; a code: bits 0-3 its length, bits 4-12 its symbol; a primary slot that leads to
// the second level: bit 15, bits 0-3 the index bits there, bits 4-14 where its entries begin.
constexpr uint32_t kLink = 0x8000;

struct Shared {  // what a workgroup (a stream) keeps in LDS: 2048 + 256 + 5120 + 1536 + 352 + 64 + 64 + 4096 + 16 = 13552 B
  alignas(16) uint8_t win[kWindow];
  uint8_t line[kLine];
  uint16_t lit[kLitTable];
  uint16_t dist[kDistTable];
  uint8_t lens[32 + kMaxSymbols];  // the code-length code's 19, then the lengths of a block's two sets
  uint32_t count[16];
  uint32_t first[16];        // the first code of each length
  uint32_t deep[1u << kLitRoot];  // per primary slot, while a table is built: the longest code under it
  uint32_t cursor[4];        // [0]: the second level's allocation
};

struct Stream {
  const uint8_t* seg;  // the coded bytes
  uint32_t len;
  uint8_t* out;
  uint32_t need;
};

struct Walk {
  Shared& sh;
  const Stream st;
  const uint32_t lane;
  uint32_t base = 0;     // of the window
  uint64_t next = 0;     // the next byte (a multiple of 4) to enter the accumulator
  uint64_t hold = 0;     // LSB first
  uint32_t bits = 0;     // in hold (zeros behind the stream's end included)
  uint32_t o = 0;        // bytes stored
  uint32_t nline = 0;    // literals waiting in sh.line
  bool fixed_built = false;

  INFLATE_FN Walk(Shared& s, const Stream& t) : sh(s), st(t), lane(lane_id()) {}

  // ---- coded bytes
  INFLATE_FN void stage(uint32_t from) {  // from: a multiple of 4
    sync();
    base = from;
    for (uint32_t j = lane; j < kWindow; j += kLanes) sh.win[j] = (uint64_t)from + j < st.len ? st.seg[from + j] : 0;
    sync();
  }
  INFLATE_FN uint32_t word(uint64_t at) {  // bytes at .. at + 4 of the stream, zeros behind its end; at a multiple of 4
    if (at >= st.len) return 0;             // (nothing to stage: the walk ends within a few steps)
    const uint32_t i = (uint32_t)at;
    if (i - base >= kWindow) stage(i);
    uint32_t w;
    __builtin_memcpy(&w, __builtin_assume_aligned(sh.win + (i - base), 4), 4);
    return uni(w);
  }
  INFLATE_FN void fill() {  // at least 32 bits in hold
    if (bits <= 32) {
      hold |= (uint64_t)word(next) << bits;
      bits += 32;
      next += 4;
    }
  }
  INFLATE_FN uint64_t consumed() const { return next * 8 - bits; }  // bits of the stream taken so far
  INFLATE_FN bool inside() const { return consumed() <= (uint64_t)st.len * 8; }
  INFLATE_FN uint32_t peek(uint32_t n) const { return (uint32_t)hold & ((1u << n) - 1); }  // n <= 16, after fill()
  INFLATE_FN void drop(uint32_t n) { hold >>= n; bits -= n; }
  INFLATE_FN uint32_t take(uint32_t n) { const uint32_t v = peek(n); drop(n); return v; }
  INFLATE_FN void seek(uint64_t byte) {  // byte <= len
    const uint64_t at = byte & ~(uint64_t)3;
    const uint32_t skip = ((uint32_t)byte & 3) * 8;
    hold = (uint64_t)word(at) >> skip;
    bits = 32 - skip;
    next = at + 4;
  }

  // ---- output
  INFLATE_FN void flush() {  // the literals of the line, by the lanes
    if (nline == 0) return;
    sync();
    for (uint32_t j = lane; j < nline; j += kLanes) st.out[o + j] = sh.line[j];
    sync();
    o += nline;
    nline = 0;
  }
  INFLATE_FN uint32_t done() const { return o + nline; }
  INFLATE_FN void literal(uint32_t v) {  // done() < need
    if (lane == 0) sh.line[nline] = (uint8_t)v;
    if (++nline == kLine) flush();
  }

  // ---- tables
  // The decoding table of `n` code lengths at sh.lens + at: false where zlib's inflate_table refuses the set.
  INFLATE_FN bool build(uint32_t at, uint32_t n, uint16_t* tab, uint32_t root, uint32_t sub_cap, bool complete = false) {
    const uint32_t primary = 1u << root;
    sync();
    for (uint32_t j = lane; j < 16; j += kLanes) sh.count[j] = 0;
    for (uint32_t j = lane; j < primary + sub_cap; j += kLanes) tab[j] = 0;
    for (uint32_t j = lane; j < primary; j += kLanes) sh.deep[j] = 0;
    if (lane == 0) sh.cursor[0] = 0;
    sync();
    for (uint32_t j = lane; j < n; j += kLanes) add(&sh.count[sh.lens[at + j] & 15], 1);
    sync();
    // over-subscribed, incomplete: inflate_table's own test
    int32_t left = 1;
    uint32_t max = 0, code = 0;
    for (uint32_t l = 1; l <= 15; ++l) {
      const uint32_t c = uni(sh.count[l]);
      left = (left << 1) - (int32_t)c;
      if (left < 0) return false;
      if (c) max = l;
      if (lane == 0) sh.first[l] = code;
      code = (code + c) << 1;
    }
    if (complete ? left != 0 : left > 0 && max > 1) return false;
    if (max == 0) return true;  // no code at all: every slot says so
    sync();
    // a lane a length: its symbols in order get its codes in order; a code is kept bit-reversed, as the stream has it
    for (uint32_t l = 1 + lane; l <= 15; l += kLanes) {
      uint32_t c = sh.first[l];
      if (sh.count[l] == 0) continue;
      for (uint32_t s = 0; s < n; ++s) {
        if (sh.lens[at + s] != l) continue;
        uint32_t r = 0;
        for (uint32_t b = 0; b < l; ++b) r |= ((c >> b) & 1) << (l - 1 - b);
        ++c;
        const uint32_t e = l | (s << 4);
        if (l <= root) {
          for (uint32_t k = r; k < primary; k += 1u << l) tab[k] = (uint16_t)e;
        } else {
          raise(&sh.deep[r & (primary - 1)], l);
        }
      }
    }
    if (max <= root) { sync(); return true; }
    sync();
    // the second level: room per primary slot, then its codes
    for (uint32_t p = lane; p < primary; p += kLanes) {
      const uint32_t d = sh.deep[p];
      if (d == 0) continue;
      const uint32_t from = add(&sh.cursor[0], 1u << (d - root));
      if (from + (1u << (d - root)) > sub_cap) continue;
      tab[p] = (uint16_t)(kLink | (d - root) | (from << 4));
    }
    sync();
    if (uni(sh.cursor[0]) > sub_cap) return false;  // (the bound above says it cannot happen)
    for (uint32_t l = root + 1 + lane; l <= 15; l += kLanes) {
      uint32_t c = sh.first[l];
      if (sh.count[l] == 0) continue;
      for (uint32_t s = 0; s < n; ++s) {
        if (sh.lens[at + s] != l) continue;
        uint32_t r = 0;
        for (uint32_t b = 0; b < l; ++b) r |= ((c >> b) & 1) << (l - 1 - b);
        ++c;
        const uint32_t link = tab[r & (primary - 1)];
        const uint32_t sb = link & 15, from = (link >> 4) & 0x7ff;
        if (!(link & kLink) || from + (1u << sb) > sub_cap) continue;  // (a prefix-free set never comes here)
        for (uint32_t k = r >> root; k < (1u << sb); k += 1u << (l - root)) tab[primary + from + k] = (uint16_t)(l | (s << 4));
      }
    }
    sync();
    return true;
  }
  // the entry of the next code (0: none), not yet dropped; after fill()
  INFLATE_FN uint32_t lookup(const uint16_t* tab, uint32_t root) const {
    uint32_t e = uni(tab[(uint32_t)hold & ((1u << root) - 1)]);
    if (e & kLink) {
      const uint32_t sb = e & 15, from = (e >> 4) & 0x7ff;
      e = uni(tab[(1u << root) + from + (((uint32_t)hold >> root) & ((1u << sb) - 1))]);
    }
    return e;
  }

  INFLATE_FN bool fixed_tables() {
    if (fixed_built) return true;
    sync();
    for (uint32_t j = lane; j < 288; j += kLanes) sh.lens[j] = j < 144 ? 8 : j < 256 ? 9 : j < 280 ? 7 : 8;
    for (uint32_t j = lane; j < 32; j += kLanes) sh.lens[288 + j] = 5;
    sync();
    if (!build(0, 288, sh.lit, kLitRoot, kLitSub) || !build(288, 32, sh.dist, kDistRoot, kDistSub)) return false;
    fixed_built = true;
    return true;
  }

  INFLATE_FN bool dynamic_tables() {
    fixed_built = false;
    fill();
    const uint32_t nlen = take(5) + 257, ndist = take(5) + 1, ncode = take(4) + 4;
    if (!inside() || nlen > 286 || ndist > 30) return false;
    sync();
    for (uint32_t j = lane; j < 19; j += kLanes) sh.lens[j] = 0;
    sync();
    for (uint32_t j = 0; j < ncode; ++j) {
      fill();
      const uint32_t v = take(3);
      if (lane == 0) sh.lens[code_order(j)] = (uint8_t)v;
    }
    if (!inside()) return false;
    // the code-length code: at most 7 bits, so its table is a primary level alone, in the literal table's place; it must be
    // complete (zlib lets an empty one through and then finds no end-of-block code: the same refusal, nothing in between)
    if (!build(0, 19, sh.lit, 7, 0, true)) return false;
    // the lengths themselves, serially; they are kept behind the 19 (the tables are built from there)
    const uint32_t at = 32, total = nlen + ndist;
    uint32_t have = 0;
    while (have < total) {
      fill();
      const uint32_t e = uni(sh.lit[(uint32_t)hold & 127]);
      if ((e & 15) == 0) return false;
      drop(e & 15);
      const uint32_t sym = e >> 4;
      if (!inside()) return false;
      if (sym < 16) {
        if (lane == 0) sh.lens[at + have] = (uint8_t)sym;
        ++have;
        continue;
      }
      uint32_t v = 0, run;
      fill();
      if (sym == 16) {
        if (have == 0) return false;
        sync();
        v = uni(sh.lens[at + have - 1]);
        run = 3 + take(2);
      } else if (sym == 17) run = 3 + take(3);
      else run = 11 + take(7);
      if (!inside() || have + run > total) return false;
      sync();
      for (uint32_t j = lane; j < run; j += kLanes) sh.lens[at + have + j] = (uint8_t)v;
      have += run;
    }
    sync();
    if (uni(sh.lens[at + 256]) == 0) return false;  // no end-of-block code
    return build(at, nlen, sh.lit, kLitRoot, kLitSub) && build(at + nlen, ndist, sh.dist, kDistRoot, kDistSub);
  }
  static INFLATE_FN uint32_t code_order(uint32_t j) {  // 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15, 5 bits each
    const uint64_t lo = 16ull | 17ull << 5 | 18ull << 10 | 0ull << 15 | 8ull << 20 | 7ull << 25 | 9ull << 30 | 6ull << 35 | 10ull << 40 | 5ull << 45 | 11ull << 50 | 4ull << 55;
    const uint64_t hi = 12ull | 3ull << 5 | 13ull << 10 | 2ull << 15 | 14ull << 20 | 1ull << 25 | 15ull << 30;
    return j < 12 ? (uint32_t)(lo >> (5 * j)) & 31 : (uint32_t)(hi >> (5 * (j - 12))) & 31;
  }

  // ---- blocks
  INFLATE_FN bool stored() {  // false: a fault, or the input ends
    flush();
    drop(bits & 7);
    fill();
    const uint32_t n = take(16);
    const uint32_t inv = take(16);
    if (!inside() || n != (inv ^ 0xffffu)) return false;
    const uint64_t from = consumed() / 8;  // (a whole number: the accumulator holds whole bytes now)
    uint32_t k = n;
    if ((uint64_t)st.len - from < k) k = (uint32_t)(st.len - from);
    const uint32_t put = k < st.need - o ? k : st.need - o;
    for (uint32_t j = lane; j < put; j += kLanes) st.out[o + j] = st.seg[from + j];
    o += put;
    if (k < n) return false;
    seek(from + n);
    return true;
  }

  INFLATE_FN bool coded() {  // the symbols of a block up to its end-of-block code; false: a fault
    while (done() < st.need) {
      fill();
      const uint32_t e = lookup(sh.lit, kLitRoot);
      if ((e & 15) == 0) return false;
      drop(e & 15);
      const uint32_t sym = e >> 4;
      if (sym < 256) {
        if (!inside()) return false;
        literal(sym);
        continue;
      }
      if (sym == 256) return inside();
      if (sym > 285) return false;
      // length: 257 .. 264 are 3 .. 10, then four codes per extra bit, 285 is 258
      uint32_t length;
      fill();
      if (sym < 265) length = sym - 254;
      else if (sym == 285) length = 258;
      else {
        const uint32_t x = (sym - 261) >> 2;
        length = 3 + ((4 + ((sym - 265) & 3)) << x) + take(x);
      }
      fill();
      const uint32_t d = lookup(sh.dist, kDistRoot);
      if ((d & 15) == 0) return false;
      drop(d & 15);
      const uint32_t dsym = d >> 4;
      if (dsym > 29) return false;
      uint32_t distance = dsym + 1;
      if (dsym >= 4) {
        const uint32_t x = (dsym >> 1) - 1;
        fill();
        distance = 1 + ((2 + (dsym & 1)) << x) + take(x);
      }
      if (!inside()) return false;
      flush();
      if (distance > o) return false;
      const uint32_t n = length < st.need - o ? length : st.need - o;
      const uint8_t* from = st.out + (o - distance);
      uint8_t* to = st.out + o;
      if (distance >= n) {
        for (uint32_t k = lane; k < n; k += kLanes) to[k] = from[k];
      } else {  // the source runs into what this match writes: it repeats with the distance as its period
        for (uint32_t k = lane; k < n; k += kLanes) to[k] = from[k % distance];
      }
      o += n;
    }
    return true;
  }

  // the whole stream; the bytes produced
  INFLATE_FN uint32_t run() {
    stage(0);
    fill();
    const uint32_t cmf = take(8), flg = take(8);
    bool ok = inside() && (cmf & 15) == 8 && (cmf >> 4) <= 7 && ((cmf << 8) | flg) % 31 == 0 && !(flg & 0x20);
    while (ok && done() < st.need) {
      fill();
      const uint32_t last = take(1), type = take(2);
      if (!inside()) break;
      if (type == 0) ok = stored();
      else if (type == 1) ok = fixed_tables() && coded();
      else if (type == 2) ok = dynamic_tables() && coded();
      else ok = false;
      if (last) break;
    }
    flush();
    return o;
  }
};

}  // namespace inflate_core
}  // namespace ocr
