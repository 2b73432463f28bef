// Host side of the device JPEG 2000 back-end + its C-ABI entry points.
#include <algorithm>
#include <cstring>

#include "capi_common.h"
#include "j2k_stage.h"

namespace ocr {

namespace {

using PaddleOCR::j2k::Rect;
using PaddleOCR::j2k::TileComp;
namespace j2k = PaddleOCR::j2k;
static_assert(sizeof(ocr_j2k_tilecomp) == sizeof(TileComp) && offsetof(ocr_j2k_tilecomp, levels) == offsetof(TileComp, levels) &&
                  offsetof(ocr_j2k_tilecomp, step_off) == offsetof(TileComp, step_off) && offsetof(ocr_j2k_tilecomp, coeff_off) == offsetof(TileComp, coeff_off),
              "ocr_j2k_tilecomp is j2k::TileComp");

static_assert(sizeof(ocr_j2k_cblk) == sizeof(j2k::CodedBlock) && offsetof(ocr_j2k_cblk, byte_off) == offsetof(j2k::CodedBlock, byte_off) &&
                  offsetof(ocr_j2k_cblk, w) == offsetof(j2k::CodedBlock, w) && offsetof(ocr_j2k_cblk, passes) == offsetof(j2k::CodedBlock, passes),
              "ocr_j2k_cblk is j2k::CodedBlock");

size_t pad256(size_t bytes) { return (bytes + 255) & ~(size_t)255; }

// What a batch of validated frames comes to on the device: tile-components, tiles, steps, the units of every launch, and
// where each tile-component's samples lie in the planes.
struct J2kPlan {
  std::vector<J2kTc> tcs;
  std::vector<J2kTile> tiles;
  std::vector<float> steps;
  std::vector<J2kUnit> units;
  struct Src { const int32_t* from; size_t at, n; };  // a tile-component's coefficients: where they go in plane a
  std::vector<Src> src;
  std::vector<uint32_t> first_tc;  // per image: its first tile-component in tcs
  size_t samples = 0;
  J2kLaunch L;
  size_t at_steps = 0, at_tcs = 0, at_tiles = 0, at_units = 0, end = 0;  // byte offsets in the batch's data, from plane a's start

  bool build(const ocr_j2k_frame* const* imgs, int count, uint8_t* const* dst, std::string& err) {
    int max_levels = 0;
    for (int i = 0; i < count; ++i) {
      const ocr_j2k_frame& f = *imgs[i];
      first_tc.push_back((uint32_t)tcs.size());
      for (size_t t = 0; t < f.tcs_len; t += (size_t)f.ncomp) {
        J2kTile T;
        memset(&T, 0, sizeof T);
        T.ncomp = f.ncomp; T.mct = f.mct; T.prec = f.prec; T.transform = f.transform;
        for (int k = 0; k < 3; ++k) T.chan[k] = f.chan[k];
        T.img_w = f.width; T.ox = f.tcs[t].x0 - f.x0; T.oy = f.tcs[t].y0 - f.y0;
        T.dst = dst ? dst[i] : nullptr;
        for (int c = 0; c < f.ncomp; ++c) {
          const ocr_j2k_tilecomp& a = f.tcs[t + (size_t)c];
          const size_t n = (size_t)(a.x1 - a.x0) * (size_t)(a.y1 - a.y0);
          if (samples + n > ((size_t)1 << 31)) { err = "j2k batch: more samples than the device stage indexes"; return false; }
          T.tc[c] = (uint32_t)tcs.size();
          tcs.push_back(J2kTc{a.x0, a.y0, a.x1, a.y1, a.levels, f.transform, (uint32_t)samples, (uint32_t)steps.size()});
          steps.insert(steps.end(), f.steps + a.step_off, f.steps + a.step_off + 1 + 3 * (size_t)a.levels);
          src.push_back(Src{f.coeffs ? f.coeffs + a.coeff_off : nullptr, samples, n});
          samples += n;
          max_levels = std::max(max_levels, a.levels);
        }
        tiles.push_back(T);
      }
    }
    // the units: a job with L levels produces resolution r = s - (max_levels - L) at step s, so that all finish together
    L.steps.resize((size_t)max_levels);
    for (int st = 1; st <= max_levels; ++st) {
      J2kStep& S = L.steps[(size_t)st - 1];
      for (int pass = 0; pass < 2; ++pass) {
        (pass ? S.v_first : S.h_first) = (uint32_t)units.size();
        for (size_t j = 0; j < tcs.size(); ++j) {
          const J2kTc& tc = tcs[j];
          const int r = st - (max_levels - tc.levels);
          if (r < 1 || (pass && r == tc.levels)) continue;  // (the last level's columns are the finishing pass's)
          const Rect cur = j2k::res_rect(Rect{tc.x0, tc.y0, tc.x1, tc.y1}, tc.levels - r);
          const int cw = cur.x1 - cur.x0, ch = cur.y1 - cur.y0;
          if (cw < 1 || ch < 1) continue;
          if (!pass) {
            for (int q = 0; q < ch; q += kJ2kRows)
              for (int p = 0; p < cw; p += kJ2kRowWin - 2 * kJ2kHalo) units.push_back(J2kUnit{(uint32_t)j, r, p, q});
          } else {
            for (int q = 0; q < ch; q += kJ2kColWin - 2 * kJ2kHalo)
              for (int p = 0; p < cw; p += kJ2kCols) units.push_back(J2kUnit{(uint32_t)j, r, p, q});
          }
        }
        (pass ? S.v_count : S.h_count) = (uint32_t)units.size() - (pass ? S.v_first : S.h_first);
      }
    }
    L.fin_first = (uint32_t)units.size();
    for (size_t j = 0; j < tiles.size(); ++j) {
      const J2kTc& tc = tcs[tiles[j].tc[0]];
      for (int q = 0; q < tc.y1 - tc.y0; q += kJ2kColWin - 2 * kJ2kHalo)
        for (int p = 0; p < tc.x1 - tc.x0; p += kJ2kCols) units.push_back(J2kUnit{(uint32_t)j, tc.levels, p, q});
    }
    L.fin_count = (uint32_t)units.size() - L.fin_first;
    at_steps = pad256(samples * 4); at_tcs = at_steps + pad256(steps.size() * 4); at_tiles = at_tcs + pad256(tcs.size() * sizeof(J2kTc));
    at_units = at_tiles + pad256(tiles.size() * sizeof(J2kTile)); end = at_units + pad256(units.size() * sizeof(J2kUnit));
    return true;
  }
  // the descriptors into the staging buffer whose byte 0 is byte `origin` of the batch's data
  void descriptors(uint8_t* stage, size_t origin) const {
    memcpy(stage + at_steps - origin, steps.data(), steps.size() * 4);
    memcpy(stage + at_tcs - origin, tcs.data(), tcs.size() * sizeof(J2kTc));
    memcpy(stage + at_tiles - origin, tiles.data(), tiles.size() * sizeof(J2kTile));
    memcpy(stage + at_units - origin, units.data(), units.size() * sizeof(J2kUnit));
  }
  void point(J2kScratch& sc) {
    L.batch.a = (const int32_t*)sc.data.p;
    L.batch.b = sc.rows.p;
    L.batch.r = sc.recon.p;
    L.batch.steps = (const float*)(sc.data.p + at_steps);
    L.batch.tcs = (const J2kTc*)(sc.data.p + at_tcs);
    L.batch.tiles = (const J2kTile*)(sc.data.p + at_tiles);
    L.batch.units = (const J2kUnit*)(sc.data.p + at_units);
  }
};

}  // namespace

// host/j2k_decode.h fault_of() and device_fault(): the one statement of the rules
const char* j2k_frame_fault(const ocr_j2k_frame& f) {
  if (!f.steps || !f.coeffs) return "j2k frame: steps or coefficients are missing";
  if (const char* why = j2k::fault_of(f.width, f.height, f.x0, f.y0, f.ncomp, f.prec, f.transform, f.mct, f.chan, (const TileComp*)f.tcs, f.tcs_len, f.steps_len, f.coeffs_len))
    return why;
  return j2k::device_fault(f.width, f.height, f.ncomp, (const TileComp*)f.tcs, f.tcs_len);
}

void j2k_relaunch(const J2kLaunch& L, hipStream_t s) { launch_j2k(L.batch, L.steps.data(), (int)L.steps.size(), L.fin_first, L.fin_count, s); }

int j2k_decode_async(const ocr_j2k_frame* const* imgs, int count, uint8_t* const* dst, J2kScratch& sc, hipStream_t s, std::string& err, J2kLaunch* launched) {
  for (int i = 0; i < count; ++i) {
    if (!imgs[i]) { err = "null j2k frame"; return OCR_ERR_ARG; }
    if (const char* fault = j2k_frame_fault(*imgs[i])) { err = fault; return OCR_ERR_ARG; }
  }
  J2kPlan P;
  if (!P.build(imgs, count, dst, err)) return OCR_ERR_ARG;
  J2kLaunch& L = P.L;
  L.bytes = P.end;
  if (!sc.data.ensure(P.end + 256, err) || !sc.rows.ensure(P.samples + 64, err) || !sc.recon.ensure(P.samples + 64, err)) return OCR_ERR_DEVICE;
  if (!sc.stage.reserve(P.end + 256, err)) return OCR_ERR_DEVICE;
  parallel_copy(P.src.size(), P.samples * 4, [&](size_t i) { memcpy(sc.stage.p + P.src[i].at * 4, P.src[i].from, P.src[i].n * 4); });  // descriptors -> pinned memory
  P.descriptors(sc.stage.p, 0);
  P.point(sc);
  if (!sc.stage.upload(sc.data.p, P.end, s, err)) { err = "j2k descriptor upload failed"; return OCR_ERR_DEVICE; }
  j2k_relaunch(L, s);
  if (hipGetLastError() != hipSuccess) { err = "j2k sample kernels failed to launch"; return OCR_ERR_DEVICE; }
  if (launched) *launched = std::move(L);
  return OCR_OK;
}

// host/j2k_decode.h fault_of(), device_fault() and coded_fault(): the one statement of the rules
const char* j2k_coded_fault(const ocr_j2k_coded& c) {
  const ocr_j2k_frame& f = c.frame;
  if (!f.steps) return "j2k frame: steps or coefficients are missing";
  if (f.coeffs) return "j2k coded: a coded frame carries no coefficients";
  if (c.bytes_len && !c.bytes) return "j2k coded: the byte pool is missing";
  if (const char* why = j2k::fault_of(f.width, f.height, f.x0, f.y0, f.ncomp, f.prec, f.transform, f.mct, f.chan, (const TileComp*)f.tcs, f.tcs_len, f.steps_len, f.coeffs_len))
    return why;
  if (const char* why = j2k::device_fault(f.width, f.height, f.ncomp, (const TileComp*)f.tcs, f.tcs_len)) return why;
  return j2k::coded_fault((const TileComp*)f.tcs, f.tcs_len, (const j2k::CodedBlock*)c.cblks, c.cblks_len, c.bytes_len);
}

hipError_t j2k_t1_relaunch(const J2kLaunch& L, hipStream_t s) {
  const hipError_t e = hipMemsetAsync((void*)L.batch.a, 0, L.plane_bytes, s);
  if (e != hipSuccess) return e;
  launch_j2k_t1(L.blocks, L.nblocks, L.pool, (int32_t*)L.batch.a, s);
  return hipGetLastError();
}

int j2k_coded_decode_async(const ocr_j2k_coded* const* imgs, int count, uint8_t* const* dst, J2kScratch& sc, hipStream_t s, std::string& err, J2kLaunch* launched,
                           bool pixels) {
  std::vector<const ocr_j2k_frame*> frames((size_t)count);
  size_t nblocks = 0, nbytes = 0;
  for (int i = 0; i < count; ++i) {
    if (!imgs[i]) { err = "null j2k frame"; return OCR_ERR_ARG; }
    if (const char* fault = j2k_coded_fault(*imgs[i])) { err = fault; return OCR_ERR_ARG; }
    frames[(size_t)i] = &imgs[i]->frame;
    nblocks += imgs[i]->cblks_len;
    nbytes += imgs[i]->bytes_len;
  }
  if (nbytes > 0xffffffffu || nblocks > 0x7fffffffu) { err = "j2k batch: more coded blocks or bytes than the device stage indexes"; return OCR_ERR_ARG; }
  J2kPlan P;
  if (!P.build(frames.data(), count, dst, err)) return OCR_ERR_ARG;
  // the batch's blocks, the costly ones first: a block's time goes with passes * samples, and the last workgroups to start
  // should be short ones
  std::vector<J2kT1Block> blocks;
  blocks.reserve(nblocks);
  size_t pool_at = 0;
  for (int i = 0; i < count; ++i) {
    const ocr_j2k_coded& c = *imgs[i];
    for (size_t b = 0; b < c.cblks_len; ++b) {
      const ocr_j2k_cblk& k = c.cblks[b];
      const J2kTc& tc = P.tcs[P.first_tc[(size_t)i] + k.tc];
      blocks.push_back(J2kT1Block{tc.plane + k.at, (uint32_t)(tc.x1 - tc.x0), (uint32_t)(pool_at + k.byte_off), k.byte_len, k.w, k.h, k.orient, k.numbps, k.passes, 0});
    }
    pool_at += c.bytes_len;
  }
  std::stable_sort(blocks.begin(), blocks.end(), [](const J2kT1Block& a, const J2kT1Block& b) { return (int)a.passes * a.w * a.h > (int)b.passes * b.w * b.h; });
  const size_t at_blocks = P.end, at_pool = at_blocks + pad256(blocks.size() * sizeof(J2kT1Block)), end = at_pool + pad256(nbytes);
  J2kLaunch& L = P.L;
  L.plane_bytes = P.samples * 4;
  L.upload_at = P.at_steps;
  L.bytes = end - L.upload_at;
  L.nblocks = (uint32_t)blocks.size();
  if (!sc.data.ensure(end + 256, err) || !sc.rows.ensure(P.samples + 64, err) || !sc.recon.ensure(P.samples + 64, err)) return OCR_ERR_DEVICE;
  if (!sc.stage.reserve(L.bytes + 256, err)) return OCR_ERR_DEVICE;
  P.descriptors(sc.stage.p, L.upload_at);
  if (!blocks.empty()) memcpy(sc.stage.p + at_blocks - L.upload_at, blocks.data(), blocks.size() * sizeof(J2kT1Block));
  pool_at = at_pool - L.upload_at;
  for (int i = 0; i < count; ++i) {
    if (imgs[i]->bytes_len) memcpy(sc.stage.p + pool_at, imgs[i]->bytes, imgs[i]->bytes_len);
    pool_at += imgs[i]->bytes_len;
  }
  P.point(sc);
  L.blocks = (const J2kT1Block*)(sc.data.p + at_blocks);
  L.pool = sc.data.p + at_pool;
  if (!sc.stage.upload(sc.data.p + L.upload_at, L.bytes, s, err)) { err = "j2k descriptor upload failed"; return OCR_ERR_DEVICE; }
  if (j2k_t1_relaunch(L, s) != hipSuccess) { err = "j2k tier-1 kernel failed to launch"; return OCR_ERR_DEVICE; }
  if (pixels) {
    j2k_relaunch(L, s);
    if (hipGetLastError() != hipSuccess) { err = "j2k sample kernels failed to launch"; return OCR_ERR_DEVICE; }
  }
  if (launched) *launched = std::move(L);
  return OCR_OK;
}

}  // namespace ocr

using namespace ocr;

namespace {

struct J2kRoute {
  using Frame = ocr_j2k_frame;
  using Scratch = J2kScratch;
  using Launch = J2kLaunch;
  static const char* fault(const Frame& f) { return j2k_frame_fault(f); }
  static int rows(const Frame& f) { return f.height; }
  static int cols(const Frame& f) { return f.width; }
  static int decode(const Frame* const* frames, int count, uint8_t* const* dst, Scratch& sc, std::string& err, Launch* L) {
    return j2k_decode_async(frames, count, dst, sc, nullptr, err, L);
  }
  static uint8_t* uploaded(Scratch& sc, const Launch&) { return sc.data.p; }
  static void pixels(Scratch&, const Launch& L) { j2k_relaunch(L, nullptr); }
};

// the coded route: upload (of what follows plane a), tier-1, pixel stage
struct J2kCodedRoute {
  using Frame = ocr_j2k_coded;
  using Scratch = J2kScratch;
  using Launch = J2kLaunch;
  static const char* fault(const Frame& c) { return j2k_coded_fault(c); }
  static int rows(const Frame& c) { return c.frame.height; }
  static int cols(const Frame& c) { return c.frame.width; }
  static int decode(const Frame* const* coded, int count, uint8_t* const* dst, Scratch& sc, std::string& err, Launch* L) {
    return j2k_coded_decode_async(coded, count, dst, sc, nullptr, err, L);
  }
  static uint8_t* uploaded(Scratch& sc, const Launch& L) { return sc.data.p + L.upload_at; }
  static hipError_t middle(Scratch&, const Launch& L) { return j2k_t1_relaunch(L, nullptr); }
  static void pixels(Scratch&, const Launch& L) { j2k_relaunch(L, nullptr); }
};

}  // namespace

extern "C" int ocr_j2k_decode(const ocr_j2k_frame* frame, int device_id, uint8_t* bgr, size_t cap) { return decode_frame<J2kRoute>(frame, device_id, bgr, cap); }

extern "C" int ocr_j2k_time(const ocr_j2k_frame* frame, int device_id, int iters, double ms[2]) {
  if (!frame || !ms || iters <= 0) return fail(OCR_ERR_ARG, "null argument");
  return time_frames<J2kRoute>(&frame, 1, device_id, iters, ms);
}

extern "C" int ocr_j2k_time_batch(const ocr_j2k_frame* const* frames, int count, int device_id, int iters, double ms[2]) {
  if (!frames || count < 1 || !ms || iters <= 0) return fail(OCR_ERR_ARG, "null argument");
  return time_frames<J2kRoute>(frames, count, device_id, iters, ms);
}

extern "C" int ocr_j2k_tier1(const ocr_j2k_coded* coded, int device_id, int32_t* coeffs, size_t cap) {
  if (!coded || !coeffs) return fail(OCR_ERR_ARG, "null argument");
  if (const char* fault = j2k_coded_fault(*coded)) return fail(OCR_ERR_ARG, fault);
  const ocr_j2k_frame& f = coded->frame;
  if (f.coeffs_len > cap) return fail(OCR_ERR_CAPACITY, "output buffer too small");
  int rc = ocr_rt_init(device_id);
  if (rc) return rc;
  J2kScratch sc;
  J2kLaunch L;
  std::string err;
  rc = j2k_coded_decode_async(&coded, 1, nullptr, sc, nullptr, err, &L, false);
  if (rc) return fail(rc, err);
  // plane a holds the tile-components one after another, in the order of tcs
  std::vector<int32_t> plane(L.plane_bytes / 4);
  CAPI_HIP(hipStreamSynchronize(nullptr));
  CAPI_HIP(g_memcpy(plane.data(), L.batch.a, L.plane_bytes, hipMemcpyDeviceToHost));
  std::fill(coeffs, coeffs + f.coeffs_len, 0);
  size_t at = 0;
  for (size_t t = 0; t < f.tcs_len; ++t) {
    const size_t n = (size_t)(f.tcs[t].x1 - f.tcs[t].x0) * (size_t)(f.tcs[t].y1 - f.tcs[t].y0);
    memcpy(coeffs + f.tcs[t].coeff_off, plane.data() + at, n * 4);
    at += n;
  }
  return OCR_OK;
}

extern "C" int ocr_j2k_decode_coded(const ocr_j2k_coded* coded, int device_id, uint8_t* bgr, size_t cap) {
  return decode_frame<J2kCodedRoute>(coded, device_id, bgr, cap);
}

extern "C" int ocr_j2k_time_coded(const ocr_j2k_coded* coded, int device_id, int iters, double ms[3]) {
  if (!coded || !ms || iters <= 0) return fail(OCR_ERR_ARG, "null argument");
  return time_frames3<J2kCodedRoute>(&coded, 1, device_id, iters, ms);
}

extern "C" int ocr_j2k_time_coded_batch(const ocr_j2k_coded* const* coded, int count, int device_id, int iters, double ms[3]) {
  if (!coded || count < 1 || !ms || iters <= 0) return fail(OCR_ERR_ARG, "null argument");
  return time_frames3<J2kCodedRoute>(coded, count, device_id, iters, ms);
}
