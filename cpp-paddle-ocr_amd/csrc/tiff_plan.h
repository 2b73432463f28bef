// Everything about a batch of TIFF frames that is arithmetic, with nothing of HIP in it (capi_tiff.hip does the device calls
// around it; host/tiff_plan_check.cpp runs it alone): the rules of a frame on this side of the ABI, the image descriptors of
// the pixel stage, and the plan of a coded batch - where each frame's chunks and bytes lie, and the chunk records in the order
// of the launch.  A further compression is a Route, a row in coded_fault, a record maker and a row in build().
#pragma once
#include <algorithm>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "../host/tiff_decode.h"  // the rules of a coded frame and the scans of its streams, stated once
#include "../../include/ocr_hip.h"
#include "tiff_desc.h"

namespace ocr {
namespace tiff_plan {

namespace tiff = PaddleOCR::tiff;

static_assert(sizeof(ocr_tiff_chunk) == sizeof(tiff::Chunk) && offsetof(ocr_tiff_chunk, byte_off) == offsetof(tiff::Chunk, byte_off) &&
                  offsetof(ocr_tiff_chunk, byte_len) == offsetof(tiff::Chunk, byte_len) && offsetof(ocr_tiff_chunk, rows) == offsetof(tiff::Chunk, rows),
              "ocr_tiff_chunk is tiff::Chunk");
static_assert(offsetof(ocr_tiff_fax, coded) == 0, "a fax descriptor starts with its coded frame");

// The ways a coded frame's chunks are expanded on the device.  The frames of every route are handed about as ocr_tiff_coded;
// those of kFax are the first member of an ocr_tiff_fax each.
enum Route { kCoded, kDeflate, kFax };

inline uint32_t t4_options(Route route, const ocr_tiff_coded& c) { return route == kFax ? ((const ocr_tiff_fax*)&c)->t4_options : 0; }

inline size_t pad256(size_t bytes) { return (bytes + 255) & ~(size_t)255; }

// host/tiff_decode.h fault(), rule for rule; with_data: the frame carries its expanded chunks (a coded frame does not)
inline const char* tiff_fault(const ocr_tiff_frame& f, tiff::Geometry& g, bool with_data = true) {
  if (f.width <= 0 || f.height <= 0 || (long)f.width * f.height > (64L << 20)) return "tiff frame: width and height must be positive and at most 64 Mpixel together";
  if (f.bits_per_sample != 1 && f.bits_per_sample != 2 && f.bits_per_sample != 4 && f.bits_per_sample != 8 && f.bits_per_sample != 16)
    return "tiff frame: bits per sample must be 1, 2, 4, 8 or 16";
  if (f.samples_per_pixel < 1 || f.samples_per_pixel > 16) return "tiff frame: samples per pixel must be 1 .. 16";
  if (f.planar != 1 && f.planar != 2) return "tiff frame: planar must be 1 or 2";
  if (f.predictor != 1 && f.predictor != 2) return "tiff frame: predictor must be 1 or 2";
  if ((f.big_endian | 1) != 1 || (f.premultiply | 1) != 1) return "tiff frame: big_endian and premultiply must be 0 or 1";
  const int ph = f.photometric, bits = f.bits_per_sample, spp = f.samples_per_pixel;
  if (ph != 0 && ph != 1 && ph != 2 && ph != 3 && ph != 5) return "tiff frame: photometric must be 0, 1, 2, 3 or 5";
  g.colour = ph == 2 ? 3 : ph == 5 ? 4 : 1;
  if (spp < g.colour) return "tiff frame: fewer samples per pixel than the photometric needs";
  if (bits < 8 && (ph == 2 || ph == 5 || spp != 1 || f.predictor != 1 || f.planar != 1)) return "tiff frame: 1, 2 and 4 bits: grey or palette, one sample, no predictor, chunky";
  if (ph == 3 && (bits > 8 || f.planar != 1)) return "tiff frame: palette: at most 8 bits, chunky";
  if (ph == 5 && (bits != 8 || f.planar != 1)) return "tiff frame: CMYK: 8 bits, chunky";
  if (f.planar == 2 && ph != 2 && spp < 2) return "tiff frame: planar 2: RGB, or grey with extra samples";
  if (f.premultiply && (spp <= g.colour || !(ph == 2 || (ph <= 1 && f.planar == 2)))) return "tiff frame: premultiply: RGB with alpha, or grey with alpha in planes";
  if (f.tile_width <= 0 || f.tile_height <= 0 || (long)f.tile_width * f.tile_height > (64L << 20))
    return "tiff frame: tile_width and tile_height must be positive and at most 64 Mpixel together";
  g.used = g.colour + f.premultiply;
  g.planes = f.planar == 2 ? spp : 1;
  g.across = (int)(((long)f.width + f.tile_width - 1) / f.tile_width);
  g.down = (int)(((long)f.height + f.tile_height - 1) / f.tile_height);
  g.row_bytes = ((size_t)f.tile_width * (f.planar == 2 ? 1 : spp) * bits + 7) / 8;  // <= 2^26 * 32
  g.chunk_bytes = g.row_bytes * (size_t)f.tile_height;                              // <= 2^26 * 32 + 2^26
  g.total = g.chunk_bytes * (size_t)g.across * g.down * g.planes;                   // < 2^32 * 2^26 * 2^4
  if (g.total > ((size_t)1 << 30)) return "tiff frame: the chunks at their nominal size exceed 1 GiB";
  if (with_data && (!f.data || f.data_len < g.total)) return "tiff frame: data_len is less than the chunks at their nominal size";
  return nullptr;
}

inline tiff::Frame host_frame(const ocr_tiff_frame& f) {
  tiff::Frame h;
  h.width = f.width; h.height = f.height; h.photometric = f.photometric; h.bits = f.bits_per_sample; h.samples = f.samples_per_pixel;
  h.planar = f.planar; h.predictor = f.predictor; h.big_endian = f.big_endian; h.premultiply = f.premultiply;
  h.tile_width = f.tile_width; h.tile_height = f.tile_height;
  return h;
}

// Why a coded frame is refused, nullptr when it is sound: tiff_fault(), then the host's rules for the route (kCoded:
// tiff::coded_fault_of with the extent scan of every chunk; kDeflate: tiff::deflate_fault_of, which looks at no stream; kFax:
// tiff::fax_structure_fault), then the device bounds - and for a fax frame behind them the widest chunk the device expansion
// takes and only then the walk of every stream (tiff::fax_fault_of).
inline const char* coded_fault(Route route, const ocr_tiff_coded& c, tiff::Geometry& g) {
  const ocr_tiff_frame& f = c.frame;
  if (f.data) return "tiff coded: a coded frame carries no expanded chunks";
  if (const char* why = tiff_fault(f, g, false)) return why;
  const tiff::Frame h = host_frame(f);
  const tiff::Chunk* chunks = (const tiff::Chunk*)c.chunks;
  const uint32_t t4 = t4_options(route, c);
  tiff::Geometry hg;
  const char* why = route == kCoded     ? tiff::coded_fault_of(h, c.compression, chunks, c.chunks_len, c.bytes, c.bytes_len, hg)
                    : route == kDeflate ? tiff::deflate_fault_of(h, c.compression, chunks, c.chunks_len, c.bytes, c.bytes_len, hg)
                                        : tiff::fax_structure_fault(h, c.compression, t4, chunks, c.chunks_len, c.bytes_len, hg);
  if (why) return why;
  if (c.chunks_len > tiff::kMaxDeviceChunks || g.total > tiff::kMaxDeviceBytes) return "tiff coded: beyond the device bounds (2^20 chunks, 512 MiB at their nominal size)";
  if (route != kFax) return nullptr;
  static_assert(tiff::kMaxFaxDeviceWidth == kTiffFaxMaxWidth, "the host sends what the lists of the kernel have room for");
  if (f.tile_width > kTiffFaxMaxWidth) return "tiff fax: a chunk wider than the device expansion takes (8192 pixels)";
  return tiff::fax_fault_of(h, c.compression, t4, chunks, c.chunks_len, c.bytes, c.bytes_len, hg);
}

// What the pixel stage launches: id[first[k]] .. + count[k] are the frames of kind k, units[k] their units.
struct Kinds {
  int first[kTiffKinds] = {}, count[kTiffKinds] = {};
  unsigned long long units[kTiffKinds] = {};
};

inline int kind_of(const ocr_tiff_frame& f) { return f.bits_per_sample < 8 ? 0 : f.bits_per_sample == 8 ? 1 : 2; }
inline const ocr_tiff_frame& frame_of(const ocr_tiff_frame& f) { return f; }
inline const ocr_tiff_frame& frame_of(const ocr_tiff_coded& c) { return c.frame; }

// The descriptors of validated frames (F: ocr_tiff_frame or ocr_tiff_coded) ordered by the kernel that takes them, the units of
// a kind numbered through its frames; frame i's chunks lie at data + off[i] (device).  Fills K.
template <class F>
std::vector<TiffImageDesc> describe(const F* const* imgs, int count, const std::vector<tiff::Geometry>& geo, const std::vector<size_t>& off,
                                    uint8_t* const* dst, const uint8_t* data, Kinds& K) {
  for (int i = 0; i < count; ++i) K.count[kind_of(frame_of(*imgs[i]))]++;
  for (int k = 1; k < kTiffKinds; ++k) K.first[k] = K.first[k - 1] + K.count[k - 1];
  int next[kTiffKinds];
  std::copy(K.first, K.first + kTiffKinds, next);
  std::vector<TiffImageDesc> id((size_t)count);
  for (int i = 0; i < count; ++i) {
    const ocr_tiff_frame& f = frame_of(*imgs[i]);
    const tiff::Geometry& g = geo[i];
    const int kind = kind_of(f);
    TiffImageDesc& d = id[next[kind]++];
    memset(&d, 0, sizeof d);
    d.data = data + off[i];
    d.bgr = dst ? dst[i] : nullptr;
    d.first_unit = K.units[kind];
    d.chunk_bytes = g.chunk_bytes;
    d.plane_bytes = f.planar == 2 ? g.chunk_bytes * (size_t)g.across * g.down : 0;
    d.row_bytes = g.row_bytes;
    d.width = f.width; d.height = f.height; d.tile_width = f.tile_width; d.tile_height = f.tile_height; d.across = g.across; d.down = g.down;
    d.bits = f.bits_per_sample; d.samples = f.samples_per_pixel; d.used = g.used;
    d.mode = f.photometric == 3 ? TIFF_PALETTE : f.photometric == 5 ? TIFF_CMYK : f.photometric == 2 ? TIFF_RGB : f.planar == 2 ? TIFF_GREY_PLANES : TIFF_GREY;
    d.predictor = f.predictor; d.big_endian = f.big_endian; d.invert = f.photometric == 0; d.premultiply = f.premultiply;
    d.lanes_per_row = tiff_lanes_per_row(std::min(f.tile_width, f.width));
    d.rows_per_unit = 64 / d.lanes_per_row;
    d.units_per_chunk = (unsigned)((std::min(f.tile_height, f.height) + d.rows_per_unit - 1) / d.rows_per_unit);
    K.units[kind] += (unsigned long long)g.across * g.down * d.units_per_chunk;  // <= chunks * rows of a chunk: < 2^27
    for (int k = 0; k < 256; ++k) d.palette[k] = (uint32_t)f.palette[4 * k] | ((uint32_t)f.palette[4 * k + 1] << 8) | ((uint32_t)f.palette[4 * k + 2] << 16);
  }
  return id;
}

// ---- the plan of a coded batch
struct Whose { int frame; uint32_t chunk; };

struct Plan {
  Route route = kCoded;
  std::vector<tiff::Geometry> geo;   // per frame, from coded_fault (the caller fills it before build())
  std::vector<size_t> off, pool_at;  // per frame: of its expanded chunks in the batch's, of its bytes in the batch's pool
  size_t bytes = 0;                  // of the expanded chunks, every frame padded to 256
  size_t pool = 0, nchunks = 0;
  std::vector<Whose> whose;          // per record in the order of the launch: the frame and the chunk it came from
  std::vector<size_t> first_chunk;   // per frame: its first chunk's number in the order of the batch
  std::vector<uint64_t> words;       // the records in the order of the launch, in the route's record type
  size_t record_bytes = 0;           // of all of them
  uint32_t lzw = 0, runs = 0;        // kCoded: records[0 .. lzw) are the LZW chunks, the `runs` behind them the others
  size_t at_pool = 0, coded_bytes = 0;  // the upload: the records padded to 256, then the pool padded to 256
  const void* records() const { return words.data(); }
};

inline bool chunks_fit_a_launch(size_t nchunks) { return nchunks <= 0x7fffffffu; }  // one workgroup a chunk

// the makers: record (frame i, chunk k) of the batch
inline TiffChunkDesc make_record(const Plan& P, const ocr_tiff_coded& c, int i, uint32_t k, TiffChunkDesc*) {
  const tiff::Geometry& g = P.geo[i];
  return TiffChunkDesc{P.pool_at[i] + c.chunks[k].byte_off, P.off[i] + k * g.chunk_bytes, c.chunks[k].byte_len, (uint32_t)(c.chunks[k].rows * g.row_bytes),
                       (uint32_t)g.chunk_bytes, (uint32_t)c.compression};
}
inline InflateDesc make_record(const Plan& P, const ocr_tiff_coded& c, int i, uint32_t k, InflateDesc*) {
  const tiff::Geometry& g = P.geo[i];
  return InflateDesc{P.pool_at[i] + c.chunks[k].byte_off, P.off[i] + k * g.chunk_bytes, c.chunks[k].byte_len, (uint32_t)(c.chunks[k].rows * g.row_bytes),
                     (uint32_t)g.chunk_bytes};
}
inline TiffFaxDesc make_record(const Plan& P, const ocr_tiff_coded& c, int i, uint32_t k, TiffFaxDesc*) {
  const tiff::Geometry& g = P.geo[i];
  return TiffFaxDesc{P.pool_at[i] + c.chunks[k].byte_off, P.off[i] + k * g.chunk_bytes, c.chunks[k].byte_len, c.chunks[k].rows,
                     (uint32_t)g.chunk_bytes, (uint32_t)c.frame.tile_width, (uint32_t)c.compression, t4_options(kFax, c)};
}
template <class Rec>
void make_records(Plan& P, const ocr_tiff_coded* const* imgs) {
  static_assert(sizeof(Rec) % sizeof(uint64_t) == 0 && alignof(Rec) <= alignof(uint64_t), "records lie in 8-byte words");
  P.record_bytes = P.whose.size() * sizeof(Rec);
  P.words.resize(P.record_bytes / sizeof(uint64_t));
  Rec* r = (Rec*)P.words.data();
  for (size_t n = 0; n < P.whose.size(); ++n) new (r + n) Rec(make_record(P, *imgs[P.whose[n].frame], P.whose[n].frame, P.whose[n].chunk, (Rec*)nullptr));
}

// The plan of `count` validated frames of one route, P.route and P.geo given.  false: more chunks than a launch has
// workgroups (nothing but nchunks is then filled).  The order of the launch: the long streams first, so that they do not form
// the tail, chunks of equal length in the order of the batch; kCoded: the LZW chunks so, then the others so.
inline bool build(Plan& P, const ocr_tiff_coded* const* imgs, int count) {
  P.off.resize((size_t)count); P.pool_at.resize((size_t)count); P.first_chunk.resize((size_t)count);
  for (int i = 0; i < count; ++i) {
    P.off[i] = P.bytes;
    P.pool_at[i] = P.pool;
    P.first_chunk[i] = P.nchunks;
    P.bytes += pad256(P.geo[i].total);
    P.nchunks += imgs[i]->chunks_len;
    P.pool += imgs[i]->bytes_len;
  }
  if (!chunks_fit_a_launch(P.nchunks)) return false;
  P.whose.reserve(P.nchunks);
  for (int pass = 0; pass < 2; ++pass) {
    for (int i = 0; i < count; ++i) {
      if ((P.route != kCoded || imgs[i]->compression == 5) != (pass == 0)) continue;
      for (size_t k = 0; k < imgs[i]->chunks_len; ++k) P.whose.push_back(Whose{i, (uint32_t)k});
    }
    if (pass == 0 && P.route == kCoded) P.lzw = (uint32_t)P.whose.size();
  }
  if (P.route == kCoded) P.runs = (uint32_t)P.whose.size() - P.lzw;
  auto longer = [&](const Whose& a, const Whose& b) { return imgs[a.frame]->chunks[a.chunk].byte_len > imgs[b.frame]->chunks[b.chunk].byte_len; };
  std::stable_sort(P.whose.begin(), P.whose.begin() + P.lzw, longer);
  std::stable_sort(P.whose.begin() + P.lzw, P.whose.end(), longer);
  if (P.route == kCoded) make_records<TiffChunkDesc>(P, imgs);
  else if (P.route == kDeflate) make_records<InflateDesc>(P, imgs);
  else make_records<TiffFaxDesc>(P, imgs);
  P.at_pool = pad256(P.record_bytes);
  P.coded_bytes = P.at_pool + pad256(P.pool);
  return true;
}

// A Deflate batch after its launch, produced[n] the bytes record n's stream gave: the record of the first chunk, in the order
// of the batch, whose stream fell short of what its rows need; P.whose.size() where none did.
inline size_t first_short(const Plan& P, const uint32_t* produced) {
  const InflateDesc* r = (const InflateDesc*)P.records();
  size_t bad = P.whose.size(), bad_at = P.nchunks;
  for (size_t n = 0; n < P.whose.size(); ++n) {
    const size_t at = P.first_chunk[P.whose[n].frame] + P.whose[n].chunk;
    if (produced[n] != r[n].need && at < bad_at) { bad = n; bad_at = at; }
  }
  return bad;
}

// the refusal of a Deflate batch whose record `bad` fell short; ids[i]: frame i's place in the caller's batch, else i
inline std::string short_text(const Plan& P, size_t bad, const int* ids) {
  const Whose w = P.whose[bad];
  return "deflate: a chunk's stream does not hold the bytes its rows need (frame " + std::to_string(ids ? ids[w.frame] : w.frame) + ", chunk " + std::to_string(w.chunk) + ")";
}

}  // namespace tiff_plan
}  // namespace ocr
