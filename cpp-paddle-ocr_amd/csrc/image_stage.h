// What the image-format back-ends (JPEG, PNG, BMP / PNM) and the pipeline's staging slots share on the host side: the pinned
// staging buffer, the threaded host copy into it, the two-phase timing loop and the single-frame decode.
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

}  // namespace ocr
