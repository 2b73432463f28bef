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

size_t pad256(size_t bytes) { return (bytes + 255) & ~(size_t)255; }

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
  std::vector<J2kTc> tcs;
  std::vector<J2kTile> tiles;
  std::vector<float> steps;
  struct Src { const int32_t* from; size_t at, n; };  // a tile-component's coefficients: where they go in plane a
  std::vector<Src> src;
  size_t samples = 0;
  int max_levels = 0;
  for (int i = 0; i < count; ++i) {
    if (!imgs[i]) { err = "null j2k frame"; return OCR_ERR_ARG; }
    if (const char* fault = j2k_frame_fault(*imgs[i])) { err = fault; return OCR_ERR_ARG; }
    const ocr_j2k_frame& f = *imgs[i];
    for (size_t t = 0; t < f.tcs_len; t += (size_t)f.ncomp) {
      J2kTile T;
      memset(&T, 0, sizeof T);
      T.ncomp = f.ncomp; T.mct = f.mct; T.prec = f.prec; T.transform = f.transform;
      for (int k = 0; k < 3; ++k) T.chan[k] = f.chan[k];
      T.img_w = f.width; T.ox = f.tcs[t].x0 - f.x0; T.oy = f.tcs[t].y0 - f.y0;
      T.dst = dst[i];
      for (int c = 0; c < f.ncomp; ++c) {
        const ocr_j2k_tilecomp& a = f.tcs[t + (size_t)c];
        const size_t n = (size_t)(a.x1 - a.x0) * (size_t)(a.y1 - a.y0);
        if (samples + n > ((size_t)1 << 31)) { err = "j2k batch: more samples than the device stage indexes"; return OCR_ERR_ARG; }
        T.tc[c] = (uint32_t)tcs.size();
        tcs.push_back(J2kTc{a.x0, a.y0, a.x1, a.y1, a.levels, f.transform, (uint32_t)samples, (uint32_t)steps.size()});
        steps.insert(steps.end(), f.steps + a.step_off, f.steps + a.step_off + 1 + 3 * (size_t)a.levels);
        src.push_back(Src{f.coeffs + a.coeff_off, samples, n});
        samples += n;
        max_levels = std::max(max_levels, a.levels);
      }
      tiles.push_back(T);
    }
  }
  // the units: a job with L levels produces resolution r = s - (max_levels - L) at step s, so that all finish together
  std::vector<J2kUnit> units;
  J2kLaunch L;
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
  const size_t at_steps = pad256(samples * 4), at_tcs = at_steps + pad256(steps.size() * 4), at_tiles = at_tcs + pad256(tcs.size() * sizeof(J2kTc)),
               at_units = at_tiles + pad256(tiles.size() * sizeof(J2kTile)), bytes = at_units + pad256(units.size() * sizeof(J2kUnit));
  L.bytes = bytes;
  if (!sc.data.ensure(bytes + 256, err) || !sc.rows.ensure(samples + 64, err) || !sc.recon.ensure(samples + 64, err)) return OCR_ERR_DEVICE;
  if (!sc.stage.reserve(bytes + 256, err)) return OCR_ERR_DEVICE;
  parallel_copy(src.size(), samples * 4, [&](size_t i) { memcpy(sc.stage.p + src[i].at * 4, src[i].from, src[i].n * 4); });  // descriptors -> pinned memory
  memcpy(sc.stage.p + at_steps, steps.data(), steps.size() * 4);
  memcpy(sc.stage.p + at_tcs, tcs.data(), tcs.size() * sizeof(J2kTc));
  memcpy(sc.stage.p + at_tiles, tiles.data(), tiles.size() * sizeof(J2kTile));
  memcpy(sc.stage.p + at_units, units.data(), units.size() * sizeof(J2kUnit));
  L.batch.a = (const int32_t*)sc.data.p;
  L.batch.b = sc.rows.p;
  L.batch.r = sc.recon.p;
  L.batch.steps = (const float*)(sc.data.p + at_steps);
  L.batch.tcs = (const J2kTc*)(sc.data.p + at_tcs);
  L.batch.tiles = (const J2kTile*)(sc.data.p + at_tiles);
  L.batch.units = (const J2kUnit*)(sc.data.p + at_units);
  if (!sc.stage.upload(sc.data.p, bytes, s, err)) { err = "j2k descriptor upload failed"; return OCR_ERR_DEVICE; }
  j2k_relaunch(L, s);
  if (hipGetLastError() != hipSuccess) { err = "j2k sample kernels failed to launch"; return OCR_ERR_DEVICE; }
  if (launched) *launched = std::move(L);
  return OCR_OK;
}

}  // namespace ocr

using namespace ocr;

namespace {

int time_batch(const ocr_j2k_frame* const* frames, int count, int device_id, int iters, double ms[2]) {
  for (int i = 0; i < count; ++i) {
    if (!frames[i]) return fail(OCR_ERR_ARG, "null argument");
    if (const char* fault = j2k_frame_fault(*frames[i])) return fail(OCR_ERR_ARG, fault);
  }
  int rc = ocr_rt_init(device_id);
  if (rc) return rc;
  std::vector<DevBuf<uint8_t>> out((size_t)count);
  std::vector<uint8_t*> dst((size_t)count);
  std::string err;
  for (int i = 0; i < count; ++i) {
    if (!out[i].ensure((size_t)frames[i]->width * frames[i]->height * 3, err)) return fail(OCR_ERR_DEVICE, err);
    dst[i] = out[i].p;
  }
  J2kScratch sc;
  J2kLaunch L;
  rc = j2k_decode_async(frames, count, dst.data(), sc, nullptr, err, &L);  // uploads, and the first (untimed) launches
  if (rc) return fail(rc, err);
  return time_phases(iters, ms, [&] { return hipMemcpyAsync(sc.data.p, sc.stage.p, L.bytes, hipMemcpyHostToDevice, nullptr); },
                     [&] { j2k_relaunch(L, nullptr); return hipSuccess; });
}

}  // namespace

extern "C" int ocr_j2k_decode(const ocr_j2k_frame* frame, int device_id, uint8_t* bgr, size_t cap) {
  if (!frame || !bgr) return fail(OCR_ERR_ARG, "null argument");
  // (the descriptor first: a bad one is an argument error wherever the call is made)
  if (const char* fault = j2k_frame_fault(*frame)) return fail(OCR_ERR_ARG, fault);
  const size_t bytes = (size_t)frame->width * frame->height * 3;
  if (bytes > cap) return fail(OCR_ERR_CAPACITY, "output buffer too small");
  int rc = ocr_rt_init(device_id);
  if (rc) return rc;
  J2kScratch sc;
  return decode_one(bytes, bgr, [&](uint8_t* const* dst, std::string& err) { return j2k_decode_async(&frame, 1, dst, sc, nullptr, err); });
}

extern "C" int ocr_j2k_time(const ocr_j2k_frame* frame, int device_id, int iters, double ms[2]) {
  if (!frame || !ms || iters <= 0) return fail(OCR_ERR_ARG, "null argument");
  return time_batch(&frame, 1, device_id, iters, ms);
}

extern "C" int ocr_j2k_time_batch(const ocr_j2k_frame* const* frames, int count, int device_id, int iters, double ms[2]) {
  if (!frames || count < 1 || !ms || iters <= 0) return fail(OCR_ERR_ARG, "null argument");
  return time_batch(frames, count, device_id, iters, ms);
}
