// Host side of the device TIFF back-end + its C-ABI entry points.
#include <algorithm>
#include <cstring>

#include "../host/tiff_decode.h"  // coded_fault_of and the extent scans: the rules of a coded frame, stated once
#include "capi_common.h"
#include "tiff_stage.h"

namespace ocr {

namespace {

namespace tiff = PaddleOCR::tiff;

static_assert(sizeof(ocr_tiff_chunk) == sizeof(tiff::Chunk) && offsetof(ocr_tiff_chunk, byte_off) == offsetof(tiff::Chunk, byte_off) &&
                  offsetof(ocr_tiff_chunk, byte_len) == offsetof(tiff::Chunk, byte_len) && offsetof(ocr_tiff_chunk, rows) == offsetof(tiff::Chunk, rows),
              "ocr_tiff_chunk is tiff::Chunk");

size_t pad256(size_t bytes) { return (bytes + 255) & ~(size_t)255; }

// host/tiff_decode.h Geometry: what follows from a (sound) descriptor
struct TiffGeometry {
  int across = 0, down = 0, planes = 1, colour = 1, used = 1;
  size_t row_bytes = 0, chunk_bytes = 0, total = 0;
};

// host/tiff_decode.h fault(), rule for rule; with_data: the frame carries its expanded chunks (a coded frame does not)
const char* tiff_fault(const ocr_tiff_frame& f, TiffGeometry& g, bool with_data = true) {
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

// host/tiff_decode.h coded_fault(): fault(), the records and the extent scan of every chunk, and the device bounds
const char* tiff_coded_fault_of(const ocr_tiff_coded& c, TiffGeometry& g) {
  const ocr_tiff_frame& f = c.frame;
  if (f.data) return "tiff coded: a coded frame carries no expanded chunks";
  if (const char* why = tiff_fault(f, g, false)) return why;
  tiff::Frame h;
  h.width = f.width; h.height = f.height; h.photometric = f.photometric; h.bits = f.bits_per_sample; h.samples = f.samples_per_pixel;
  h.planar = f.planar; h.predictor = f.predictor; h.big_endian = f.big_endian; h.premultiply = f.premultiply;
  h.tile_width = f.tile_width; h.tile_height = f.tile_height;
  tiff::Geometry hg;
  if (const char* why = tiff::coded_fault_of(h, c.compression, (const tiff::Chunk*)c.chunks, c.chunks_len, c.bytes, c.bytes_len, hg)) return why;
  if (c.chunks_len > tiff::kMaxDeviceChunks || g.total > tiff::kMaxDeviceBytes) return "tiff coded: beyond the device bounds (2^20 chunks, 512 MiB at their nominal size)";
  return nullptr;
}

// host/tiff_decode.h deflate_fault_of(): fault(), the records, the device bounds; no stream is looked at
const char* tiff_deflate_fault_of(const ocr_tiff_coded& c, TiffGeometry& g) {
  const ocr_tiff_frame& f = c.frame;
  if (f.data) return "tiff coded: a coded frame carries no expanded chunks";
  if (const char* why = tiff_fault(f, g, false)) return why;
  tiff::Frame h;
  h.width = f.width; h.height = f.height; h.photometric = f.photometric; h.bits = f.bits_per_sample; h.samples = f.samples_per_pixel;
  h.planar = f.planar; h.predictor = f.predictor; h.big_endian = f.big_endian; h.premultiply = f.premultiply;
  h.tile_width = f.tile_width; h.tile_height = f.tile_height;
  tiff::Geometry hg;
  if (const char* why = tiff::deflate_fault_of(h, c.compression, (const tiff::Chunk*)c.chunks, c.chunks_len, c.bytes, c.bytes_len, hg)) return why;
  if (c.chunks_len > tiff::kMaxDeviceChunks || g.total > tiff::kMaxDeviceBytes) return "tiff coded: beyond the device bounds (2^20 chunks, 512 MiB at their nominal size)";
  return nullptr;
}

// host/tiff_decode.h fax_fault_of(): fault(), the coding's rules, the records and the walk of every chunk; the device bounds
const char* tiff_fax_fault_of(const ocr_tiff_fax& x, TiffGeometry& g) {
  const ocr_tiff_coded& c = x.coded;
  const ocr_tiff_frame& f = c.frame;
  if (f.data) return "tiff coded: a coded frame carries no expanded chunks";
  if (const char* why = tiff_fault(f, g, false)) return why;
  tiff::Frame h;
  h.width = f.width; h.height = f.height; h.photometric = f.photometric; h.bits = f.bits_per_sample; h.samples = f.samples_per_pixel;
  h.planar = f.planar; h.predictor = f.predictor; h.big_endian = f.big_endian; h.premultiply = f.premultiply;
  h.tile_width = f.tile_width; h.tile_height = f.tile_height;
  tiff::Geometry hg;
  // the rules that need no stream first, the device bounds among them; then the walk of every chunk
  if (const char* why = tiff::fax_structure_fault(h, c.compression, x.t4_options, (const tiff::Chunk*)c.chunks, c.chunks_len, c.bytes_len, hg)) return why;
  if (c.chunks_len > tiff::kMaxDeviceChunks || g.total > tiff::kMaxDeviceBytes) return "tiff coded: beyond the device bounds (2^20 chunks, 512 MiB at their nominal size)";
  static_assert(tiff::kMaxFaxDeviceWidth == kTiffFaxMaxWidth, "the host sends what the lists of the kernel have room for");
  if (f.tile_width > kTiffFaxMaxWidth) return "tiff fax: a chunk wider than the device expansion takes (8192 pixels)";
  return tiff::fax_fault_of(h, c.compression, x.t4_options, (const tiff::Chunk*)c.chunks, c.chunks_len, c.bytes, c.bytes_len, hg);
}

int kind_of(const ocr_tiff_frame& f) { return f.bits_per_sample < 8 ? 0 : f.bits_per_sample == 8 ? 1 : 2; }

// The descriptors of validated frames ordered by the kernel that takes them, the units of a kind numbered through its
// frames; frame i's chunks lie at data + off[i].  Fills L's counts and units.
std::vector<TiffImageDesc> describe(const ocr_tiff_frame* const* imgs, int count, const std::vector<TiffGeometry>& geo, const std::vector<size_t>& off,
                                    uint8_t* const* dst, const uint8_t* data, TiffLaunch& L) {
  for (int i = 0; i < count; ++i) L.count[kind_of(*imgs[i])]++;
  for (int k = 1; k < kTiffKinds; ++k) L.first[k] = L.first[k - 1] + L.count[k - 1];
  int next[kTiffKinds];
  std::copy(L.first, L.first + kTiffKinds, next);
  std::vector<TiffImageDesc> id((size_t)count);
  for (int i = 0; i < count; ++i) {
    const ocr_tiff_frame& f = *imgs[i];
    const TiffGeometry& g = geo[i];
    const int kind = kind_of(f);
    TiffImageDesc& d = id[next[kind]++];
    memset(&d, 0, sizeof d);
    d.data = data + off[i];
    d.bgr = dst ? dst[i] : nullptr;
    d.first_unit = L.units[kind];
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
    L.units[kind] += (unsigned long long)g.across * g.down * d.units_per_chunk;  // <= chunks * rows of a chunk: < 2^27
    for (int k = 0; k < 256; ++k) d.palette[k] = (uint32_t)f.palette[4 * k] | ((uint32_t)f.palette[4 * k + 1] << 8) | ((uint32_t)f.palette[4 * k + 2] << 16);
  }
  return id;
}

}  // namespace

const char* tiff_frame_fault(const ocr_tiff_frame& f) {
  TiffGeometry g;
  return tiff_fault(f, g);
}

void tiff_relaunch(const TiffScratch& sc, const TiffLaunch& L, hipStream_t s) {
  for (int k = 0; k < kTiffKinds; ++k)
    if (L.count[k] > 0) launch_tiff(k, sc.id.p + L.first[k], L.count[k], L.units[k], s);
}

int tiff_decode_async(const ocr_tiff_frame* const* imgs, int count, uint8_t* const* dst, TiffScratch& sc, hipStream_t s, std::string& err,
                      TiffLaunch* launched) {
  std::vector<size_t> off((size_t)count);
  std::vector<TiffGeometry> geo((size_t)count);
  size_t bytes = 0;
  TiffLaunch L;
  for (int i = 0; i < count; ++i) {
    if (!imgs[i]) { err = "null tiff frame"; return OCR_ERR_ARG; }
    if (const char* fault = tiff_fault(*imgs[i], geo[i])) { err = fault; return OCR_ERR_ARG; }
    off[i] = bytes;
    bytes += pad256(geo[i].total);
  }
  L.bytes = bytes;
  if (!sc.data.ensure(bytes + 256, err) || !sc.id.ensure((size_t)count, err)) return OCR_ERR_DEVICE;
  if (!sc.stage.reserve(bytes, err)) return OCR_ERR_DEVICE;
  parallel_copy((size_t)count, bytes, [&](size_t i) { memcpy(sc.stage.p + off[i], imgs[i]->data, geo[i].total); });  // chunks -> pinned memory
  const std::vector<TiffImageDesc> id = describe(imgs, count, geo, off, dst, sc.data.p, L);
  if (!sc.stage.upload(sc.data.p, bytes, s, err) ||
      hipMemcpyAsync(sc.id.p, id.data(), id.size() * sizeof(TiffImageDesc), hipMemcpyHostToDevice, s) != hipSuccess) {
    err = "tiff chunks upload failed";
    return OCR_ERR_DEVICE;
  }
  tiff_relaunch(sc, L, s);
  if (launched) *launched = L;
  if (hipGetLastError() != hipSuccess) { err = "tiff pixel kernels failed to launch"; return OCR_ERR_DEVICE; }
  return OCR_OK;
}

const char* tiff_coded_fault(const ocr_tiff_coded& c) {
  TiffGeometry g;
  return tiff_coded_fault_of(c, g);
}

void tiff_expand_relaunch(const TiffScratch& sc, const TiffLaunch& L, hipStream_t s) { launch_tiff_expand(L.chunks, L.lzw, L.runs, L.pool, sc.data.p, s); }

int tiff_coded_decode_async(const ocr_tiff_coded* const* imgs, int count, uint8_t* const* dst, TiffScratch& sc, hipStream_t s, std::string& err,
                            TiffLaunch* launched, bool pixels) {
  std::vector<size_t> off((size_t)count), pool_at((size_t)count);
  std::vector<TiffGeometry> geo((size_t)count);
  std::vector<const ocr_tiff_frame*> frames((size_t)count);
  size_t bytes = 0, nchunks = 0, pool = 0;
  TiffLaunch L;
  for (int i = 0; i < count; ++i) {
    if (!imgs[i]) { err = "null tiff frame"; return OCR_ERR_ARG; }
    if (const char* fault = tiff_coded_fault_of(*imgs[i], geo[i])) { err = fault; return OCR_ERR_ARG; }
    frames[i] = &imgs[i]->frame;
    off[i] = bytes;
    pool_at[i] = pool;
    bytes += pad256(geo[i].total);
    nchunks += imgs[i]->chunks_len;
    pool += imgs[i]->bytes_len;
  }
  if (nchunks > 0x7fffffffu) { err = "tiff batch: more chunks than a launch has workgroups"; return OCR_ERR_ARG; }
  // the batch's chunks: the LZW ones, then the others; within each the long streams first, so that they do not form the tail
  std::vector<TiffChunkDesc> cd;
  cd.reserve(nchunks);
  for (int pass = 0; pass < 2; ++pass) {
    for (int i = 0; i < count; ++i) {
      const ocr_tiff_coded& c = *imgs[i];
      if ((c.compression == 5) != (pass == 0)) continue;
      for (size_t k = 0; k < c.chunks_len; ++k)
        cd.push_back(TiffChunkDesc{pool_at[i] + c.chunks[k].byte_off, off[i] + k * geo[i].chunk_bytes, c.chunks[k].byte_len,
                                   (uint32_t)(c.chunks[k].rows * geo[i].row_bytes), (uint32_t)geo[i].chunk_bytes, (uint32_t)c.compression});
    }
    if (pass == 0) L.lzw = (uint32_t)cd.size();
  }
  L.runs = (uint32_t)cd.size() - L.lzw;
  auto longer = [](const TiffChunkDesc& a, const TiffChunkDesc& b) { return a.byte_len > b.byte_len; };
  std::stable_sort(cd.begin(), cd.begin() + L.lzw, longer);
  std::stable_sort(cd.begin() + L.lzw, cd.end(), longer);
  const size_t at_pool = pad256(cd.size() * sizeof(TiffChunkDesc)), coded_bytes = at_pool + pad256(pool);
  L.bytes = coded_bytes;
  if (!sc.data.ensure(bytes + 256, err) || !sc.coded.ensure(coded_bytes + 256, err) || !sc.id.ensure((size_t)count, err)) return OCR_ERR_DEVICE;
  if (!sc.stage.reserve(coded_bytes, err)) return OCR_ERR_DEVICE;
  if (!cd.empty()) memcpy(sc.stage.p, cd.data(), cd.size() * sizeof(TiffChunkDesc));
  parallel_copy((size_t)count, pool, [&](size_t i) { if (imgs[i]->bytes_len) memcpy(sc.stage.p + at_pool + pool_at[i], imgs[i]->bytes, imgs[i]->bytes_len); });
  L.chunks = (const TiffChunkDesc*)sc.coded.p;
  L.pool = sc.coded.p + at_pool;
  const std::vector<TiffImageDesc> id = describe(frames.data(), count, geo, off, dst, sc.data.p, L);
  if (!sc.stage.upload(sc.coded.p, coded_bytes, s, err) ||
      hipMemcpyAsync(sc.id.p, id.data(), id.size() * sizeof(TiffImageDesc), hipMemcpyHostToDevice, s) != hipSuccess) {
    err = "tiff coded chunks upload failed";
    return OCR_ERR_DEVICE;
  }
  tiff_expand_relaunch(sc, L, s);
  if (hipGetLastError() != hipSuccess) { err = "tiff expansion kernels failed to launch"; return OCR_ERR_DEVICE; }
  if (pixels) {
    tiff_relaunch(sc, L, s);
    if (hipGetLastError() != hipSuccess) { err = "tiff pixel kernels failed to launch"; return OCR_ERR_DEVICE; }
  }
  if (launched) *launched = L;
  return OCR_OK;
}

const char* tiff_fax_fault(const ocr_tiff_fax& c) {
  TiffGeometry g;
  return tiff_fax_fault_of(c, g);
}

void tiff_fax_relaunch(const TiffScratch& sc, const TiffLaunch& L, hipStream_t s) { launch_tiff_fax(L.fax, L.nfax, L.pool, sc.data.p, s); }

int tiff_fax_decode_async(const ocr_tiff_fax* const* imgs, int count, uint8_t* const* dst, TiffScratch& sc, hipStream_t s, std::string& err,
                          TiffLaunch* launched, bool pixels) {
  std::vector<size_t> off((size_t)count), pool_at((size_t)count);
  std::vector<TiffGeometry> geo((size_t)count);
  std::vector<const ocr_tiff_frame*> frames((size_t)count);
  size_t bytes = 0, nchunks = 0, pool = 0;
  TiffLaunch L;
  for (int i = 0; i < count; ++i) {
    if (!imgs[i]) { err = "null tiff frame"; return OCR_ERR_ARG; }
    if (const char* fault = tiff_fax_fault_of(*imgs[i], geo[i])) { err = fault; return OCR_ERR_ARG; }
    frames[i] = &imgs[i]->coded.frame;
    off[i] = bytes;
    pool_at[i] = pool;
    bytes += pad256(geo[i].total);
    nchunks += imgs[i]->coded.chunks_len;
    pool += imgs[i]->coded.bytes_len;
  }
  if (nchunks > 0x7fffffffu) { err = "tiff batch: more chunks than a launch has workgroups"; return OCR_ERR_ARG; }
  // the batch's chunks, the long streams first, so that they do not form the tail
  std::vector<TiffFaxDesc> cd;
  cd.reserve(nchunks);
  for (int i = 0; i < count; ++i) {
    const ocr_tiff_coded& c = imgs[i]->coded;
    for (size_t k = 0; k < c.chunks_len; ++k)
      cd.push_back(TiffFaxDesc{pool_at[i] + c.chunks[k].byte_off, off[i] + k * geo[i].chunk_bytes, c.chunks[k].byte_len, c.chunks[k].rows,
                               (uint32_t)geo[i].chunk_bytes, (uint32_t)c.frame.tile_width, (uint32_t)c.compression, imgs[i]->t4_options});
  }
  std::stable_sort(cd.begin(), cd.end(), [](const TiffFaxDesc& a, const TiffFaxDesc& b) { return a.byte_len > b.byte_len; });
  L.nfax = (uint32_t)cd.size();
  const size_t at_pool = pad256(cd.size() * sizeof(TiffFaxDesc)), coded_bytes = at_pool + pad256(pool);
  L.bytes = coded_bytes;
  if (!sc.data.ensure(bytes + 256, err) || !sc.coded.ensure(coded_bytes + 256, err) || !sc.id.ensure((size_t)count, err)) return OCR_ERR_DEVICE;
  if (!sc.stage.reserve(coded_bytes, err)) return OCR_ERR_DEVICE;
  if (!cd.empty()) memcpy(sc.stage.p, cd.data(), cd.size() * sizeof(TiffFaxDesc));
  parallel_copy((size_t)count, pool, [&](size_t i) { if (imgs[i]->coded.bytes_len) memcpy(sc.stage.p + at_pool + pool_at[i], imgs[i]->coded.bytes, imgs[i]->coded.bytes_len); });
  L.fax = (const TiffFaxDesc*)sc.coded.p;
  L.pool = sc.coded.p + at_pool;
  const std::vector<TiffImageDesc> id = describe(frames.data(), count, geo, off, dst, sc.data.p, L);
  if (!sc.stage.upload(sc.coded.p, coded_bytes, s, err) ||
      hipMemcpyAsync(sc.id.p, id.data(), id.size() * sizeof(TiffImageDesc), hipMemcpyHostToDevice, s) != hipSuccess) {
    err = "tiff fax chunks upload failed";
    return OCR_ERR_DEVICE;
  }
  tiff_fax_relaunch(sc, L, s);
  if (hipGetLastError() != hipSuccess) { err = "tiff fax expansion kernel failed to launch"; return OCR_ERR_DEVICE; }
  if (pixels) {
    tiff_relaunch(sc, L, s);
    if (hipGetLastError() != hipSuccess) { err = "tiff pixel kernels failed to launch"; return OCR_ERR_DEVICE; }
  }
  if (launched) *launched = L;
  return OCR_OK;
}

const char* tiff_deflate_fault(const ocr_tiff_coded& c) {
  TiffGeometry g;
  return tiff_deflate_fault_of(c, g);
}

int tiff_inflate_relaunch(TiffScratch& sc, const TiffLaunch& L, hipStream_t s) {
  launch_inflate(L.streams, L.nstreams, L.pool, sc.data.p, sc.produced.p, s);
  if (hipGetLastError() != hipSuccess) return OCR_ERR_DEVICE;
  if (L.nstreams && hipMemcpyAsync(sc.counts.p, sc.produced.p, (size_t)L.nstreams * 4, hipMemcpyDeviceToHost, s) != hipSuccess) return OCR_ERR_DEVICE;
  return hipStreamSynchronize(s) == hipSuccess ? OCR_OK : OCR_ERR_DEVICE;
}

int tiff_deflate_decode_async(const ocr_tiff_coded* const* imgs, int count, uint8_t* const* dst, TiffScratch& sc, hipStream_t s, std::string& err,
                              TiffLaunch* launched, bool pixels, uint32_t* const* produced, const int* ids) {
  std::vector<size_t> off((size_t)count), pool_at((size_t)count);
  std::vector<TiffGeometry> geo((size_t)count);
  std::vector<const ocr_tiff_frame*> frames((size_t)count);
  size_t bytes = 0, nchunks = 0, pool = 0;
  TiffLaunch L;
  for (int i = 0; i < count; ++i) {
    if (!imgs[i]) { err = "null tiff frame"; return OCR_ERR_ARG; }
    if (const char* fault = tiff_deflate_fault_of(*imgs[i], geo[i])) { err = fault; return OCR_ERR_ARG; }
    frames[i] = &imgs[i]->frame;
    off[i] = bytes;
    pool_at[i] = pool;
    bytes += pad256(geo[i].total);
    nchunks += imgs[i]->chunks_len;
    pool += imgs[i]->bytes_len;
  }
  if (nchunks > 0x7fffffffu) { err = "tiff batch: more chunks than a launch has workgroups"; return OCR_ERR_ARG; }
  // the batch's streams, the long ones first, so that they do not form the tail; whose[k]: the frame and chunk of record k
  struct Whose { int frame; uint32_t chunk; };
  std::vector<uint32_t> order;
  std::vector<InflateDesc> sd;
  std::vector<Whose> whose;
  order.reserve(nchunks); sd.reserve(nchunks); whose.reserve(nchunks);
  for (int i = 0; i < count; ++i) {
    const ocr_tiff_coded& c = *imgs[i];
    for (size_t k = 0; k < c.chunks_len; ++k) {
      order.push_back((uint32_t)sd.size());
      sd.push_back(InflateDesc{pool_at[i] + c.chunks[k].byte_off, off[i] + k * geo[i].chunk_bytes, c.chunks[k].byte_len,
                               (uint32_t)(c.chunks[k].rows * geo[i].row_bytes), (uint32_t)geo[i].chunk_bytes});
      whose.push_back(Whose{i, (uint32_t)k});
    }
  }
  std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return sd[a].byte_len > sd[b].byte_len; });
  std::vector<InflateDesc> sorted(sd.size());
  for (size_t k = 0; k < order.size(); ++k) sorted[k] = sd[order[k]];
  L.nstreams = (uint32_t)sorted.size();
  const size_t at_pool = pad256(sorted.size() * sizeof(InflateDesc)), coded_bytes = at_pool + pad256(pool);
  L.bytes = coded_bytes;
  if (!sc.data.ensure(bytes + 256, err) || !sc.coded.ensure(coded_bytes + 256, err) || !sc.id.ensure((size_t)count, err) || !sc.produced.ensure(sorted.size() + 1, err)) return OCR_ERR_DEVICE;
  if (!sc.stage.reserve(coded_bytes, err) || !sc.counts.reserve((sorted.size() + 1) * 4, err)) return OCR_ERR_DEVICE;
  if (!sorted.empty()) memcpy(sc.stage.p, sorted.data(), sorted.size() * sizeof(InflateDesc));
  parallel_copy((size_t)count, pool, [&](size_t i) { if (imgs[i]->bytes_len) memcpy(sc.stage.p + at_pool + pool_at[i], imgs[i]->bytes, imgs[i]->bytes_len); });
  L.streams = (const InflateDesc*)sc.coded.p;
  L.pool = sc.coded.p + at_pool;
  const std::vector<TiffImageDesc> id = describe(frames.data(), count, geo, off, dst, sc.data.p, L);
  if (!sc.stage.upload(sc.coded.p, coded_bytes, s, err) ||
      hipMemcpyAsync(sc.id.p, id.data(), id.size() * sizeof(TiffImageDesc), hipMemcpyHostToDevice, s) != hipSuccess) {
    err = "tiff deflate chunks upload failed";
    return OCR_ERR_DEVICE;
  }
  if (tiff_inflate_relaunch(sc, L, s) != OCR_OK) { err = "tiff inflate kernel failed"; return OCR_ERR_DEVICE; }
  for (size_t k = 0; k < order.size(); ++k) {
    const Whose w = whose[order[k]];
    if (produced && produced[w.frame]) produced[w.frame][w.chunk] = sc.produced_host()[k];
  }
  if (pixels) {
    // the first chunk, in the order of the batch, whose stream fell short
    size_t bad = sd.size();
    for (size_t k = 0; k < order.size(); ++k)
      if (sc.produced_host()[k] != sorted[k].need && order[k] < bad) bad = order[k];
    if (bad < sd.size()) {
      const Whose w = whose[bad];
      err = "deflate: a chunk's stream does not hold the bytes its rows need (frame " + std::to_string(ids ? ids[w.frame] : w.frame) + ", chunk " + std::to_string(w.chunk) + ")";
      return OCR_ERR_ARG;
    }
    tiff_relaunch(sc, L, s);
    if (hipGetLastError() != hipSuccess) { err = "tiff pixel kernels failed to launch"; return OCR_ERR_DEVICE; }
  }
  if (launched) *launched = L;
  return OCR_OK;
}

}  // namespace ocr

using namespace ocr;

namespace {

struct TiffRoute : PlainRoute<ocr_tiff_frame, TiffScratch, TiffLaunch, tiff_frame_fault, tiff_decode_async, tiff_relaunch> {};

// the coded route: upload, expansion, pixel stage
struct TiffCodedRoute {
  using Frame = ocr_tiff_coded;
  using Scratch = TiffScratch;
  using Launch = TiffLaunch;
  static const char* fault(const Frame& c) { return tiff_coded_fault(c); }
  static int rows(const Frame& c) { return c.frame.height; }
  static int cols(const Frame& c) { return c.frame.width; }
  static int decode(const Frame* const* coded, int count, uint8_t* const* dst, Scratch& sc, std::string& err, Launch* L) {
    return tiff_coded_decode_async(coded, count, dst, sc, nullptr, err, L);
  }
  static uint8_t* uploaded(Scratch& sc, const Launch&) { return sc.coded.p; }
  static hipError_t middle(Scratch& sc, const Launch& L) { tiff_expand_relaunch(sc, L, nullptr); return hipGetLastError(); }
  static void pixels(Scratch& sc, const Launch& L) { tiff_relaunch(sc, L, nullptr); }
};

// the Deflate route: upload, the inflate launch with its read-back, pixel stage
struct TiffDeflateRoute : TiffCodedRoute {
  static const char* fault(const Frame& c) { return tiff_deflate_fault(c); }
  static int decode(const Frame* const* coded, int count, uint8_t* const* dst, Scratch& sc, std::string& err, Launch* L) {
    return tiff_deflate_decode_async(coded, count, dst, sc, nullptr, err, L);
  }
  static hipError_t middle(Scratch& sc, const Launch& L) { return tiff_inflate_relaunch(sc, L, nullptr) == OCR_OK ? hipSuccess : hipErrorUnknown; }
};

// the fax route: upload, the fax expansion, pixel stage
struct TiffFaxRoute {
  using Frame = ocr_tiff_fax;
  using Scratch = TiffScratch;
  using Launch = TiffLaunch;
  static const char* fault(const Frame& c) { return tiff_fax_fault(c); }
  static int rows(const Frame& c) { return c.coded.frame.height; }
  static int cols(const Frame& c) { return c.coded.frame.width; }
  static int decode(const Frame* const* fax, int count, uint8_t* const* dst, Scratch& sc, std::string& err, Launch* L) {
    return tiff_fax_decode_async(fax, count, dst, sc, nullptr, err, L);
  }
  static uint8_t* uploaded(Scratch& sc, const Launch&) { return sc.coded.p; }
  static hipError_t middle(Scratch& sc, const Launch& L) { tiff_fax_relaunch(sc, L, nullptr); return hipGetLastError(); }
  static void pixels(Scratch& sc, const Launch& L) { tiff_relaunch(sc, L, nullptr); }
};

}  // namespace

extern "C" int ocr_tiff_unfax(const ocr_tiff_fax* fax, int device_id, uint8_t* out, size_t cap) {
  if (!fax || !out) return fail(OCR_ERR_ARG, "null argument");
  TiffGeometry g;
  if (const char* fault = tiff_fax_fault_of(*fax, g)) return fail(OCR_ERR_ARG, fault);
  if (g.total > cap) return fail(OCR_ERR_CAPACITY, "output buffer too small");
  int rc = ocr_rt_init(device_id);
  if (rc) return rc;
  TiffScratch sc;
  std::string err;
  rc = tiff_fax_decode_async(&fax, 1, nullptr, sc, nullptr, err, nullptr, false);
  if (rc) return fail(rc, err);
  CAPI_HIP(hipStreamSynchronize(nullptr));
  CAPI_HIP(g_memcpy(out, sc.data.p, g.total, hipMemcpyDeviceToHost));
  return OCR_OK;
}

extern "C" int ocr_tiff_decode_fax(const ocr_tiff_fax* fax, int device_id, uint8_t* bgr, size_t cap) {
  return decode_frame<TiffFaxRoute>(fax, device_id, bgr, cap);
}

extern "C" int ocr_tiff_time_fax(const ocr_tiff_fax* fax, int device_id, int iters, double ms[3]) {
  if (!fax || !ms || iters <= 0) return fail(OCR_ERR_ARG, "null argument");
  return time_frames3<TiffFaxRoute>(&fax, 1, device_id, iters, ms);
}

extern "C" int ocr_tiff_time_fax_batch(const ocr_tiff_fax* const* fax, int count, int device_id, int iters, double ms[3]) {
  if (!fax || count < 1 || !ms || iters <= 0) return fail(OCR_ERR_ARG, "null argument");
  return time_frames3<TiffFaxRoute>(fax, count, device_id, iters, ms);
}

extern "C" int ocr_tiff_inflate(const ocr_tiff_coded* coded, int device_id, uint8_t* out, size_t cap, uint32_t* produced) {
  if (!coded || !out) return fail(OCR_ERR_ARG, "null argument");
  TiffGeometry g;
  if (const char* fault = tiff_deflate_fault_of(*coded, g)) return fail(OCR_ERR_ARG, fault);
  if (g.total > cap) return fail(OCR_ERR_CAPACITY, "output buffer too small");
  int rc = ocr_rt_init(device_id);
  if (rc) return rc;
  TiffScratch sc;
  std::string err;
  rc = tiff_deflate_decode_async(&coded, 1, nullptr, sc, nullptr, err, nullptr, false, produced ? &produced : nullptr);
  if (rc) return fail(rc, err);
  CAPI_HIP(g_memcpy(out, sc.data.p, g.total, hipMemcpyDeviceToHost));
  return OCR_OK;
}

extern "C" int ocr_tiff_decode_deflate(const ocr_tiff_coded* coded, int device_id, uint8_t* bgr, size_t cap) {
  return decode_frame<TiffDeflateRoute>(coded, device_id, bgr, cap);
}

extern "C" int ocr_tiff_time_deflate(const ocr_tiff_coded* coded, int device_id, int iters, double ms[3]) {
  if (!coded || !ms || iters <= 0) return fail(OCR_ERR_ARG, "null argument");
  return time_frames3<TiffDeflateRoute>(&coded, 1, device_id, iters, ms);
}

extern "C" int ocr_tiff_time_deflate_batch(const ocr_tiff_coded* const* coded, int count, int device_id, int iters, double ms[3]) {
  if (!coded || count < 1 || !ms || iters <= 0) return fail(OCR_ERR_ARG, "null argument");
  return time_frames3<TiffDeflateRoute>(coded, count, device_id, iters, ms);
}

extern "C" int ocr_tiff_expand(const ocr_tiff_coded* coded, int device_id, uint8_t* out, size_t cap) {
  if (!coded || !out) return fail(OCR_ERR_ARG, "null argument");
  TiffGeometry g;
  if (const char* fault = tiff_coded_fault_of(*coded, g)) return fail(OCR_ERR_ARG, fault);
  if (g.total > cap) return fail(OCR_ERR_CAPACITY, "output buffer too small");
  int rc = ocr_rt_init(device_id);
  if (rc) return rc;
  TiffScratch sc;
  std::string err;
  rc = tiff_coded_decode_async(&coded, 1, nullptr, sc, nullptr, err, nullptr, false);
  if (rc) return fail(rc, err);
  CAPI_HIP(hipStreamSynchronize(nullptr));
  CAPI_HIP(g_memcpy(out, sc.data.p, g.total, hipMemcpyDeviceToHost));
  return OCR_OK;
}

extern "C" int ocr_tiff_decode_coded(const ocr_tiff_coded* coded, int device_id, uint8_t* bgr, size_t cap) {
  return decode_frame<TiffCodedRoute>(coded, device_id, bgr, cap);
}

extern "C" int ocr_tiff_time_coded(const ocr_tiff_coded* coded, int device_id, int iters, double ms[3]) {
  if (!coded || !ms || iters <= 0) return fail(OCR_ERR_ARG, "null argument");
  return time_frames3<TiffCodedRoute>(&coded, 1, device_id, iters, ms);
}

extern "C" int ocr_tiff_time_coded_batch(const ocr_tiff_coded* const* coded, int count, int device_id, int iters, double ms[3]) {
  if (!coded || count < 1 || !ms || iters <= 0) return fail(OCR_ERR_ARG, "null argument");
  return time_frames3<TiffCodedRoute>(coded, count, device_id, iters, ms);
}

extern "C" int ocr_tiff_decode(const ocr_tiff_frame* frame, int device_id, uint8_t* bgr, size_t cap) { return decode_frame<TiffRoute>(frame, device_id, bgr, cap); }

extern "C" int ocr_tiff_time(const ocr_tiff_frame* frame, int device_id, int iters, double ms[2]) {
  if (!frame || !ms || iters <= 0) return fail(OCR_ERR_ARG, "null argument");
  return time_frames<TiffRoute>(&frame, 1, device_id, iters, ms);
}

extern "C" int ocr_tiff_time_batch(const ocr_tiff_frame* const* frames, int count, int device_id, int iters, double ms[2]) {
  if (!frames || count < 1 || !ms || iters <= 0) return fail(OCR_ERR_ARG, "null argument");
  return time_frames<TiffRoute>(frames, count, device_id, iters, ms);
}

// measurement aid (decode_tool --time): the device time of one plain copy KERNEL over `bytes` (16 bytes a lane, grid stride:
// launch_plain_copy), the yardstick the pixel stage's time is set against in the same run
extern "C" int ocr_dev_copy_time(void* dst, const void* src, size_t bytes, int iters, double* ms) {
  if (!dst || !src || !ms || iters <= 0 || bytes < 16 || (((uintptr_t)dst | (uintptr_t)src) & 15)) return fail(OCR_ERR_ARG, "null, unaligned or empty argument");
  launch_plain_copy(dst, src, bytes, nullptr);  // (the first launch is not timed)
  double t[2];
  const int rc = time_phases(iters, t, [&] { launch_plain_copy(dst, src, bytes, nullptr); return hipGetLastError(); }, [] { return hipSuccess; });
  if (rc == OCR_OK) *ms = t[0];
  return rc;
}
