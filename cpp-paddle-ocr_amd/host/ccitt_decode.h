// CCITT fax decoding for TIFF chunks (Compression 2 and 32771: Modified Huffman RLE; 3: T.4 / Group 3, 1-D and 2-D; 4: T.6 /
// Group 4), HIP-free: the code tables written from ITU-T T.4 / T.6 as a plain list of (code, length, run), the lookup forms
// derived from that list at compile time (the device expansion, csrc/kernels_tiff_fax.hip, holds the same tables), and walk(),
// which is both the decoder and - with no output - the scan that gives the decoder's verdict (what tiff::coded_fault is to LZW).
//
// What comes out for a well-formed chunk is what libtiff 4.3.0's tif_fax3.c produces: a white run is 0-bits and a black run
// 1-bits, whatever the photometric says (the 1-bit grey pixel stage applies MinIsWhite / MinIsBlack), rows most significant
// bit first and padded to a byte.  tests/test_tiff_fax.py pins that against TIFFReadRGBAImageOriented.
//   - Compression 2: 1-D rows with no EOL, each beginning on a byte boundary with a white run; 32771: on a 16-bit boundary
//     counted from the chunk's start
//   - Compression 3: every row behind an EOL (eleven 0s and a 1) that any number of zero fill bits may precede, whether or not
//     T4Options bit 2 announces them; T4Options bit 0 (2-D): a tag bit behind each EOL, 1 for a 1-D row and 0 for a 2-D one.
//     Whatever follows the last row (an RTC) is not looked at
//   - Compression 4: every row 2-D, the reference row of a chunk's first row all white, no EOL; an EOFB behind the last row is
//     not looked at.  The state restarts at every chunk
//   - a 1-D run is zero or more make-up codes and one terminating code; make-ups may repeat (that is how runs above 2560 are
//     coded); a run may have length 0
//   - 2-D: pass, horizontal (two complete runs, the first in the colour of a0), V0, VR1 .. VR3, VL1 .. VL3.  b1 is the first
//     changing element of the reference row to the right of a0 whose colour is opposite to a0's; a0 starts one place left of
//     the row on imaginary white, so b1 can be column 0.  A row ends when a0 reaches the width
//
// A damaged stream REFUSES the file, each class with a reason of its own (below).  That is stricter than libtiff, which
// patches a damaged row with white and goes on with a warning - the choice the LZW route made too ("an LZW code beyond the
// table refuses the file"): an OCR request is better refused than answered from a page that is part guesswork.  One rule has
// no counterpart in libtiff: a row is kept as the list of its changing elements, and a list of more than width + 1 of them -
// which only zero-length runs inside a row can make - is refused, because that is what the device expansion has room for.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

namespace PaddleOCR {
namespace ccitt {

struct Code { uint16_t bits; uint8_t len; uint16_t run; };  // the code word (its `len` low bits, sent most significant first)

// T.4 table 2 (terminating codes) and table 3a (make-up codes), white runs
constexpr Code kWhiteCodes[] = {
    {0b00110101, 8, 0},   {0b000111, 6, 1},     {0b0111, 4, 2},       {0b1000, 4, 3},       {0b1011, 4, 4},       {0b1100, 4, 5},
    {0b1110, 4, 6},       {0b1111, 4, 7},       {0b10011, 5, 8},      {0b10100, 5, 9},      {0b00111, 5, 10},     {0b01000, 5, 11},
    {0b001000, 6, 12},    {0b000011, 6, 13},    {0b110100, 6, 14},    {0b110101, 6, 15},    {0b101010, 6, 16},    {0b101011, 6, 17},
    {0b0100111, 7, 18},   {0b0001100, 7, 19},   {0b0001000, 7, 20},   {0b0010111, 7, 21},   {0b0000011, 7, 22},   {0b0000100, 7, 23},
    {0b0101000, 7, 24},   {0b0101011, 7, 25},   {0b0010011, 7, 26},   {0b0100100, 7, 27},   {0b0011000, 7, 28},   {0b00000010, 8, 29},
    {0b00000011, 8, 30},  {0b00011010, 8, 31},  {0b00011011, 8, 32},  {0b00010010, 8, 33},  {0b00010011, 8, 34},  {0b00010100, 8, 35},
    {0b00010101, 8, 36},  {0b00010110, 8, 37},  {0b00010111, 8, 38},  {0b00101000, 8, 39},  {0b00101001, 8, 40},  {0b00101010, 8, 41},
    {0b00101011, 8, 42},  {0b00101100, 8, 43},  {0b00101101, 8, 44},  {0b00000100, 8, 45},  {0b00000101, 8, 46},  {0b00001010, 8, 47},
    {0b00001011, 8, 48},  {0b01010010, 8, 49},  {0b01010011, 8, 50},  {0b01010100, 8, 51},  {0b01010101, 8, 52},  {0b00100100, 8, 53},
    {0b00100101, 8, 54},  {0b01011000, 8, 55},  {0b01011001, 8, 56},  {0b01011010, 8, 57},  {0b01011011, 8, 58},  {0b01001010, 8, 59},
    {0b01001011, 8, 60},  {0b00110010, 8, 61},  {0b00110011, 8, 62},  {0b00110100, 8, 63},
    {0b11011, 5, 64},     {0b10010, 5, 128},    {0b010111, 6, 192},   {0b0110111, 7, 256},  {0b00110110, 8, 320}, {0b00110111, 8, 384},
    {0b01100100, 8, 448}, {0b01100101, 8, 512}, {0b01101000, 8, 576}, {0b01100111, 8, 640}, {0b011001100, 9, 704}, {0b011001101, 9, 768},
    {0b011010010, 9, 832}, {0b011010011, 9, 896}, {0b011010100, 9, 960}, {0b011010101, 9, 1024}, {0b011010110, 9, 1088}, {0b011010111, 9, 1152},
    {0b011011000, 9, 1216}, {0b011011001, 9, 1280}, {0b011011010, 9, 1344}, {0b011011011, 9, 1408}, {0b010011000, 9, 1472}, {0b010011001, 9, 1536},
    {0b010011010, 9, 1600}, {0b011000, 6, 1664},  {0b010011011, 9, 1728},
};
// the same for black runs
constexpr Code kBlackCodes[] = {
    {0b0000110111, 10, 0},   {0b010, 3, 1},           {0b11, 2, 2},            {0b10, 2, 3},            {0b011, 3, 4},
    {0b0011, 4, 5},          {0b0010, 4, 6},          {0b00011, 5, 7},         {0b000101, 6, 8},        {0b000100, 6, 9},
    {0b0000100, 7, 10},      {0b0000101, 7, 11},      {0b0000111, 7, 12},      {0b00000100, 8, 13},     {0b00000111, 8, 14},
    {0b000011000, 9, 15},    {0b0000010111, 10, 16},  {0b0000011000, 10, 17},  {0b0000001000, 10, 18},  {0b00001100111, 11, 19},
    {0b00001101000, 11, 20}, {0b00001101100, 11, 21}, {0b00000110111, 11, 22}, {0b00000101000, 11, 23}, {0b00000010111, 11, 24},
    {0b00000011000, 11, 25}, {0b000011001010, 12, 26}, {0b000011001011, 12, 27}, {0b000011001100, 12, 28}, {0b000011001101, 12, 29},
    {0b000001101000, 12, 30}, {0b000001101001, 12, 31}, {0b000001101010, 12, 32}, {0b000001101011, 12, 33}, {0b000011010010, 12, 34},
    {0b000011010011, 12, 35}, {0b000011010100, 12, 36}, {0b000011010101, 12, 37}, {0b000011010110, 12, 38}, {0b000011010111, 12, 39},
    {0b000001101100, 12, 40}, {0b000001101101, 12, 41}, {0b000011011010, 12, 42}, {0b000011011011, 12, 43}, {0b000001010100, 12, 44},
    {0b000001010101, 12, 45}, {0b000001010110, 12, 46}, {0b000001010111, 12, 47}, {0b000001100100, 12, 48}, {0b000001100101, 12, 49},
    {0b000001010010, 12, 50}, {0b000001010011, 12, 51}, {0b000000100100, 12, 52}, {0b000000110111, 12, 53}, {0b000000111000, 12, 54},
    {0b000000100111, 12, 55}, {0b000000101000, 12, 56}, {0b000001011000, 12, 57}, {0b000001011001, 12, 58}, {0b000000101011, 12, 59},
    {0b000000101100, 12, 60}, {0b000001011010, 12, 61}, {0b000001100110, 12, 62}, {0b000001100111, 12, 63},
    {0b0000001111, 10, 64},   {0b000011001000, 12, 128}, {0b000011001001, 12, 192}, {0b000001011011, 12, 256}, {0b000000110011, 12, 320},
    {0b000000110100, 12, 384}, {0b000000110101, 12, 448}, {0b0000001101100, 13, 512}, {0b0000001101101, 13, 576}, {0b0000001001010, 13, 640},
    {0b0000001001011, 13, 704}, {0b0000001001100, 13, 768}, {0b0000001001101, 13, 832}, {0b0000001110010, 13, 896}, {0b0000001110011, 13, 960},
    {0b0000001110100, 13, 1024}, {0b0000001110101, 13, 1088}, {0b0000001110110, 13, 1152}, {0b0000001110111, 13, 1216}, {0b0000001010010, 13, 1280},
    {0b0000001010011, 13, 1344}, {0b0000001010100, 13, 1408}, {0b0000001010101, 13, 1472}, {0b0000001011010, 13, 1536}, {0b0000001011011, 13, 1600},
    {0b0000001100100, 13, 1664}, {0b0000001100101, 13, 1728},
};
// T.4 table 3b: the extended make-up codes, the same for both colours
constexpr Code kSharedCodes[] = {
    {0b00000001000, 11, 1792},  {0b00000001100, 11, 1856},  {0b00000001101, 11, 1920},  {0b000000010010, 12, 1984}, {0b000000010011, 12, 2048},
    {0b000000010100, 12, 2112}, {0b000000010101, 12, 2176}, {0b000000010110, 12, 2240}, {0b000000010111, 12, 2304}, {0b000000011100, 12, 2368},
    {0b000000011101, 12, 2432}, {0b000000011110, 12, 2496}, {0b000000011111, 12, 2560},
};
// T.4 table 4 / T.6 table 1: the two-dimensional modes; `run` is the mode.  kExtension is the prefix 0000001 of the extension
// codes (0000001111: uncompressed mode), which nothing here decodes - nor does libtiff
enum Mode : uint16_t { kPass = 1, kHorizontal = 2, kV0 = 3, kVR1 = 4, kVR2 = 5, kVR3 = 6, kVL1 = 7, kVL2 = 8, kVL3 = 9, kExtension = 10 };
constexpr Code kModeCodes[] = {
    {0b0001, 4, kPass}, {0b001, 3, kHorizontal}, {0b1, 1, kV0},        {0b011, 3, kVR1},     {0b000011, 6, kVR2},
    {0b0000011, 7, kVR3}, {0b010, 3, kVL1},      {0b000010, 6, kVL2},  {0b0000010, 7, kVL3}, {0b0000001, 7, kExtension},
};
constexpr int kRunBits = 13, kModeBits = 7;  // the longest code word of each kind
constexpr int kEolZeros = 11;                // an EOL is at least that many 0s and a 1

// The lookup forms.  A run table is indexed by the next 13 bits: length << 12 | run, 0 where no code word begins; a run of 64
// or more is a make-up.  The mode table by the next 7 bits: length << 4 | mode.
struct RunTable { uint16_t e[1 << kRunBits]; };
struct ModeTable { uint8_t e[1 << kModeBits]; };
template <size_t N>
constexpr void put_codes(RunTable& t, const Code (&codes)[N]) {
  for (size_t k = 0; k < N; ++k) {
    const int spare = kRunBits - codes[k].len;
    for (uint32_t j = 0; j < (1u << spare); ++j) t.e[((uint32_t)codes[k].bits << spare) + j] = (uint16_t)((codes[k].len << 12) | codes[k].run);
  }
}
constexpr RunTable make_runs(bool black) {
  RunTable t{};
  if (black) put_codes(t, kBlackCodes);
  else put_codes(t, kWhiteCodes);
  put_codes(t, kSharedCodes);
  return t;
}
constexpr ModeTable make_modes() {
  ModeTable t{};
  for (const Code& c : kModeCodes) {
    const int spare = kModeBits - c.len;
    for (uint32_t j = 0; j < (1u << spare); ++j) t.e[((uint32_t)c.bits << spare) + j] = (uint8_t)((c.len << 4) | c.run);
  }
  return t;
}
inline constexpr RunTable kWhiteRuns = make_runs(false);
inline constexpr RunTable kBlackRuns = make_runs(true);
inline constexpr ModeTable kModes = make_modes();

inline bool is_fax(int compression) { return compression == 2 || compression == 3 || compression == 4 || compression == 32771; }

// the reasons a stream is refused with
constexpr const char* kUncompressed = "fax: uncompressed mode is not decoded";
constexpr const char* kNoCode = "fax: a bit pattern that is no code word";
constexpr const char* kPasses = "fax: a run or a vertical move passes the row's width or goes left of a0";
constexpr const char* kRowShort = "fax: a row ends before its width is reached";
constexpr const char* kEnds = "fax: the stream ends before the chunk's rows are complete";
constexpr const char* kNoEol = "fax: a row of Compression 3 does not begin with an EOL";
constexpr const char* kTooMany = "fax: a row has more changing elements than its width allows";

namespace detail {

struct Bits {  // the stream, most significant bit first; behind its end it reads as zeros
  const uint8_t* s; size_t n; size_t at = 0;  // at: in bits
  size_t left() const { return at < 8 * n ? 8 * n - at : 0; }
  uint32_t peek(int k) const {  // the next k <= 16 bits
    const size_t i = at >> 3;
    uint32_t w = 0;
    for (size_t j = 0; j < 4; ++j) w = (w << 8) | (i + j < n ? s[i + j] : 0u);
    return (uint32_t)(w << (at & 7)) >> (32 - k);
  }
};

// a pattern no table has: the stream's end where fewer bits are left than the longest code word, an EOL in place of a code
// in Compression 3 (the row is over too early - or, where the row has not begun, so are the rows), else no code word
inline const char* no_code(const Bits& b, int longest, int compression, bool row_begun) {
  if (b.left() < (size_t)longest) return kEnds;
  if (b.peek(kEolZeros) == 0 && compression == 3) return row_begun ? kRowShort : kEnds;
  if (b.peek(kEolZeros) == 0 && compression == 4 && !row_begun) return kEnds;  // (an EOFB where a row should begin)
  return kNoCode;
}

// one run of a colour that may be `room` long at most: make-ups, then a terminating code.  false: *why
inline bool run(Bits& b, bool black, uint32_t room, int compression, bool row_begun, uint32_t& total, const char*& why) {
  const RunTable& t = black ? kBlackRuns : kWhiteRuns;
  total = 0;
  for (;;) {
    const uint32_t e = t.e[b.peek(kRunBits)], len = e >> 12, r = e & 0xFFF;
    if (!len) { why = no_code(b, kRunBits, compression, row_begun); return false; }
    if (len > b.left()) { why = kEnds; return false; }
    b.at += len;
    total += r;
    if (total > room) { why = kPasses; return false; }
    if (r < 64) return true;
  }
}

// bits [x0, x1) of a row to 1
inline void blacken(uint8_t* row, uint32_t x0, uint32_t x1) {
  if (x0 >= x1) return;
  const uint32_t first = x0 >> 3, last = (x1 - 1) >> 3;
  const uint8_t head = (uint8_t)(0xFF >> (x0 & 7)), tail = (uint8_t)(0xFF << (7 - ((x1 - 1) & 7)));
  if (first == last) { row[first] |= head & tail; return; }
  row[first] |= head;
  memset(row + first + 1, 0xFF, last - first - 1);
  row[last] |= tail;
}

}  // namespace detail

// A chunk's stream, `rows` rows of `width` pixels: nullptr when it is sound, else the reason.  out: the rows' bits, row_bytes
// apart, zero before the call - or nullptr for the verdict alone (the scan).  t4: T4Options (Compression 3; else 0).
// A row is its list of changing elements: the place of every colour change, the first one to black, in non-decreasing order;
// pixel x is black where an odd number of them is <= x.  Every step consumes at least one bit, so the walk ends.
inline const char* walk(const uint8_t* s, size_t n, int compression, uint32_t t4, uint32_t width, uint32_t rows, uint8_t* out, size_t row_bytes) {
  using namespace detail;
  Bits b{s, n};
  std::vector<uint32_t> lists[2];  // the row being coded and its reference row, swapped per row
  lists[0].reserve((size_t)width + 1 < 4096 ? (size_t)width + 1 : 4096);
  lists[1].reserve(lists[0].capacity());
  const char* why = nullptr;
  for (uint32_t y = 0; y < rows; ++y) {
    std::vector<uint32_t>& cur = lists[y & 1];
    const std::vector<uint32_t>& ref = lists[(y & 1) ^ 1];
    cur.clear();
    bool two_d = compression == 4;
    if (compression == 2) b.at = (b.at + 7) & ~(size_t)7;
    else if (compression == 32771) b.at = (b.at + 15) & ~(size_t)15;
    else if (compression == 3) {
      uint32_t zeros = 0;
      while (b.left() && !b.peek(1)) { ++b.at; ++zeros; }
      if (!b.left()) return kEnds;
      if (zeros < (uint32_t)kEolZeros) return kNoEol;
      ++b.at;
      if (t4 & 1) {
        if (!b.left()) return kEnds;
        two_d = !b.peek(1);
        ++b.at;
      }
    }
    auto append = [&](uint32_t x) { if (cur.size() > width) return false; cur.push_back(x); return true; };
    if (!two_d) {
      uint32_t x = 0, r;
      bool black = false, begun = false;
      while (x < width) {
        if (!run(b, black, width - x, compression, begun, r, why)) return why;
        x += r;
        if (!append(x)) return kTooMany;
        black = !black; begun = true;
      }
    } else {
      long a0 = -1;
      bool black = false;
      long bi = 0;  // into ref: the candidate for b1, of the parity that changes to the colour opposite a0's
      const long nr = (long)ref.size();
      while (a0 < (long)width) {
        const uint32_t e = kModes.e[b.peek(kModeBits)], len = e >> 4, mode = e & 15;
        if (!len) return no_code(b, kModeBits, compression, a0 >= 0);
        if (len > b.left()) return kEnds;
        if (mode == kExtension) return kUncompressed;
        b.at += len;
        const long from = a0 < 0 ? 0 : a0;
        const long b1 = bi < nr ? (long)ref[bi] : (long)width;
        if (mode == kPass) {
          a0 = bi + 1 < nr ? (long)ref[bi + 1] : (long)width;  // b2
          bi += 2;
        } else if (mode == kHorizontal) {
          uint32_t r1, r2;
          if (!run(b, black, (uint32_t)(width - from), compression, true, r1, why)) return why;
          if (!append((uint32_t)(from + r1))) return kTooMany;
          if (!run(b, !black, (uint32_t)(width - from - r1), compression, true, r2, why)) return why;
          if (!append((uint32_t)(from + r1 + r2))) return kTooMany;
          a0 = from + r1 + r2;
        } else {
          const long d = mode == kV0 ? 0 : mode <= kVR3 ? (long)mode - kV0 : -((long)mode - kVR3);
          const long a1 = b1 + d;
          if (a1 > (long)width || a1 < from) return kPasses;
          if (!append((uint32_t)a1)) return kTooMany;
          a0 = a1;
          black = !black;
          bi += d >= 0 ? 1 : -1;
        }
        while (bi < nr && (bi < 0 || (long)ref[bi] <= a0)) bi += 2;
      }
    }
    if (out) {
      uint8_t* row = out + (size_t)y * row_bytes;
      for (size_t i = 0; i < cur.size(); i += 2) blacken(row, cur[i], i + 1 < cur.size() ? cur[i + 1] : width);
    }
  }
  return nullptr;
}

}  // namespace ccitt
}  // namespace PaddleOCR
