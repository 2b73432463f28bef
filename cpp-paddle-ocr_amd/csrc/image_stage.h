// What the image-format back-ends and the pipeline's staging slots share on the host side: the pinned staging buffer, the
// threaded host copy into it, the two-phase timing loop, the single-frame decode, and the bodies of a format route's C entry
// points (decode_frame, time_frames, time_frames3 over a Route).
#pragma once
#include <algorithm>
#include <string>
#include <thread>
#include <vector>

#include "capi_common.h"
#include "stages.h"

namespace ocr {

// Pinned host memory on the way to the device.  The buffer may be refilled once `copied` has passed: upload() records it
// behind the copy, reserve() waits for it (an event that was never recorded has passed).
struct PinnedStage {
  uint8_t* p = nullptr;
  size_t cap = 0;  // bytes
  hipEvent_t copied = nullptr;
  ~PinnedStage() {
    if (p) (void)g_host_free(p);
    if (copied) (void)hipEventDestroy(copied);
  }
  bool reserve(size_t bytes, std::string& err) {
    if (!copied && hipEventCreateWithFlags(&copied, hipEventDisableTiming) != hipSuccess) { err = "hipEventCreate failed"; return false; }
    if (p && hipEventSynchronize(copied) != hipSuccess) { err = "staging event failed"; return false; }
    if (bytes <= cap) return true;
    if (p) (void)g_host_free(p);
    p = nullptr;
    cap = 0;
    if (g_host_malloc((void**)&p, bytes, hipHostMallocDefault) != hipSuccess) { err = "hipHostMalloc failed"; return false; }
    cap = bytes;
    return true;
  }
  // the first `bytes` of the buffer -> dev on `stream` (after a reserve() of at least as many)
  bool upload(void* dev, size_t bytes, hipStream_t stream, std::string& err) {
    if (hipMemcpyAsync(dev, p, bytes, hipMemcpyHostToDevice, stream) != hipSuccess) { err = "H2D copy failed"; return false; }
    if (hipEventRecord(copied, stream) != hipSuccess) { err = "hipEventRecord failed"; return false; }
    return true;
  }
};

// fn(i) for every i < count, on a few host threads when `bytes` are moved in all (one thread moves ~10 GB/s: 64 images of
// 960x960 would take 18 ms): thread t of n = min(8, max(1, bytes >> 22)) takes i = t, t + n, ...
template <class Fn>
void parallel_copy(size_t count, size_t bytes, Fn&& fn) {
  const size_t n = std::min<size_t>(8, std::max<size_t>(1, bytes >> 22));
  auto run = [&](size_t t) { for (size_t i = t; i < count; i += n) fn(i); };
  std::vector<std::thread> th;
  for (size_t t = 1; t < n; ++t) th.emplace_back(run, t);
  run(0);
  for (auto& t : th) t.join();
}

// Device time of two phases on the null stream: `iters` repetitions of first(), then of second(), between three events;
// ms[k] is the time of one repetition of phase k.  A phase returns a hipError_t.
template <class First, class Second>
int time_phases(int iters, double ms[2], First&& first, Second&& second) {
  struct Events {
    hipEvent_t e[3] = {};
    ~Events() { for (hipEvent_t x : e) if (x) (void)hipEventDestroy(x); }
  } ev;
  for (auto& e : ev.e) CAPI_HIP(hipEventCreate(&e));
  CAPI_HIP(hipEventRecord(ev.e[0], nullptr));
  for (int i = 0; i < iters; ++i) CAPI_HIP(first());
  CAPI_HIP(hipEventRecord(ev.e[1], nullptr));
  for (int i = 0; i < iters; ++i) CAPI_HIP(second());
  CAPI_HIP(hipEventRecord(ev.e[2], nullptr));
  CAPI_HIP(hipEventSynchronize(ev.e[2]));
  for (int k = 0; k < 2; ++k) {
    float t = 0;
    CAPI_HIP(hipEventElapsedTime(&t, ev.e[k], ev.e[k + 1]));
    ms[k] = (double)t / iters;
  }
  return OCR_OK;
}

// One validated frame of `bytes` output bytes into the caller's host buffer (capacity checked by the caller):
// decode(dst, err) runs the format's *_decode_async with count 1 on the null stream, dst = the address of the device pointer.
template <class Decode>
int decode_one(size_t bytes, uint8_t* bgr, Decode&& decode) {
  DevBuf<uint8_t> out;
  std::string err;
  if (!out.ensure(bytes, err)) return fail(OCR_ERR_DEVICE, err);
  uint8_t* dst = out.p;
  const int rc = decode(&dst, err);
  if (rc) return fail(rc, err);
  CAPI_HIP(g_memcpy(bgr, out.p, bytes, hipMemcpyDeviceToHost));
  return OCR_OK;
}

// ---- The C entry points of a format route (ocr_X_decode, ocr_X_time, ocr_X_time_batch) are the bodies below over a Route,
// which its capi_*.hip declares next to its *_decode_async:
//   Frame, Scratch, Launch                          the descriptor and the route's *Scratch and *Launch
//   const char* fault(const Frame&)                 why a frame is refused, nullptr when it is sound
//   int rows(const Frame&), cols(const Frame&)      of the decoded image
//   int decode(frames, count, dst, sc, err, &L)     the route's *_decode_async on the null stream
//   uint8_t* uploaded(sc, L)                        where the upload went: L.bytes from sc.stage.p
//   void pixels(sc, L)                              the pixel stage again
//   hipError_t middle(sc, L)                        a three-phase route: what runs between upload and pixel stage, again

// The routes whose frame says height and width, whose upload goes to sc.data and whose *_relaunch takes (sc, L, stream).
template <class F, class S, class L, const char* (*Fault)(const F&), int (*Decode)(const F* const*, int, uint8_t* const*, S&, hipStream_t, std::string&, L*),
          void (*Relaunch)(const S&, const L&, hipStream_t)>
struct PlainRoute {
  using Frame = F;
  using Scratch = S;
  using Launch = L;
  static const char* fault(const F& f) { return Fault(f); }
  static int rows(const F& f) { return f.height; }
  static int cols(const F& f) { return f.width; }
  static int decode(const F* const* frames, int count, uint8_t* const* dst, S& sc, std::string& err, L* launched) {
    return Decode(frames, count, dst, sc, nullptr, err, launched);
  }
  static uint8_t* uploaded(S& sc, const L&) { return sc.data.p; }
  static void pixels(S& sc, const L& launched) { Relaunch(sc, launched, nullptr); }
};

template <class Route>
int decode_frame(const typename Route::Frame* frame, int device_id, uint8_t* bgr, size_t cap) {
  if (!frame || !bgr) return fail(OCR_ERR_ARG, "null argument");
  // (the descriptor first: a bad one is an argument error wherever the call is made)
  if (const char* fault = Route::fault(*frame)) return fail(OCR_ERR_ARG, fault);
  const size_t bytes = (size_t)Route::rows(*frame) * Route::cols(*frame) * 3;
  if (bytes > cap) return fail(OCR_ERR_CAPACITY, "output buffer too small");
  const int rc = ocr_rt_init(device_id);
  if (rc) return rc;
  typename Route::Scratch sc;
  return decode_one(bytes, bgr, [&](uint8_t* const* dst, std::string& err) { return Route::decode(&frame, 1, dst, sc, err, nullptr); });
}

// A batch decoded once on the null stream into buffers of its own - the uploads, and the first (untimed) launches - and
// what the timed repetitions need of it.
template <class Route>
struct TimedBatch {
  std::vector<DevBuf<uint8_t>> out;
  typename Route::Scratch sc;
  typename Route::Launch L;
  int start(const typename Route::Frame* const* frames, int count, int device_id) {
    for (int i = 0; i < count; ++i) {
      if (!frames[i]) return fail(OCR_ERR_ARG, "null argument");
      if (const char* fault = Route::fault(*frames[i])) return fail(OCR_ERR_ARG, fault);
    }
    int rc = ocr_rt_init(device_id);
    if (rc) return rc;
    out.resize((size_t)count);
    std::vector<uint8_t*> dst((size_t)count);
    std::string err;
    for (int i = 0; i < count; ++i) {
      if (!out[i].ensure((size_t)Route::rows(*frames[i]) * Route::cols(*frames[i]) * 3, err)) return fail(OCR_ERR_DEVICE, err);
      dst[i] = out[i].p;
    }
    rc = Route::decode(frames, count, dst.data(), sc, err, &L);
    return rc ? fail(rc, err) : OCR_OK;
  }
  hipError_t upload() { return hipMemcpyAsync(Route::uploaded(sc, L), sc.stage.p, L.bytes, hipMemcpyHostToDevice, nullptr); }
};

// ms: upload, pixel stage
template <class Route>
int time_frames(const typename Route::Frame* const* frames, int count, int device_id, int iters, double ms[2]) {
  TimedBatch<Route> B;
  if (const int rc = B.start(frames, count, device_id)) return rc;
  return time_phases(iters, ms, [&] { return B.upload(); }, [&] { Route::pixels(B.sc, B.L); return hipSuccess; });
}

// ms: upload, Route::middle, pixel stage
template <class Route>
int time_frames3(const typename Route::Frame* const* frames, int count, int device_id, int iters, double ms[3]) {
  TimedBatch<Route> B;
  int rc = B.start(frames, count, device_id);
  if (rc) return rc;
  double t[2];
  rc = time_phases(iters, t, [&] { return B.upload(); }, [&] { return Route::middle(B.sc, B.L); });
  if (rc) return rc;
  ms[0] = t[0]; ms[1] = t[1];
  rc = time_phases(iters, t, [&] { Route::pixels(B.sc, B.L); return hipGetLastError(); }, [] { return hipSuccess; });
  ms[2] = t[0];
  return rc;
}

}  // namespace ocr
