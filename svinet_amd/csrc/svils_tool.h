// svils_tool.h -- the scaffold of the standalone device handles that run on a fitted model or a graph (svils_findk,
// svils_lc): one device, one stream, a fixed set of events, and device buffers tracked in two scopes -- the handle's
// lifetime and the current graph's.
//
//   svils_findk.hip   -findk: label propagation over a top-5 sparse gamma
//   svils_lc.hip      -gml / -lcstats: the link communities of a fitted model
//
// Their buffers are not the sweep handle's (svils_handle.h: dalloc): exact size, not zeroed, no slack past the end, and
// null for a count of 0.
#pragma once
#include "svils_handle.h"

namespace svils_impl {

inline uint32_t blocks(uint64_t m, uint32_t per) { return (uint32_t)((m + per - 1) / per); }

struct ToolHandle {
  enum Scope { HANDLE, GRAPH };

  int device = 0;
  hipStream_t st = nullptr;
  std::vector<hipEvent_t> ev;

  ToolHandle() = default;
  ToolHandle(const ToolHandle &) = delete;
  ToolHandle &operator=(const ToolHandle &) = delete;
  // waits for the stream, then frees both scopes, the events and the stream
  ~ToolHandle() {
    (void)hipSetDevice(device);
    if (st) (void)hipStreamSynchronize(st);
    release(GRAPH);
    release(HANDLE);
    for (hipEvent_t e : ev)
      if (e) (void)hipEventDestroy(e);
    if (st) (void)hipStreamDestroy(st);
  }

  // the stream and nev events on `device` (the current device: open_device)
  int open(int dev, int nev) {
    device = dev;
    if (hipStreamCreateWithFlags(&st, hipStreamNonBlocking) != hipSuccess) return fail(SVILS_ERR_DEVICE, "hipStreamCreate failed");
    ev.assign(nev, nullptr);
    for (hipEvent_t &e : ev)
      if (hipEventCreate(&e) != hipSuccess) return fail(SVILS_ERR_DEVICE, "hipEventCreate failed");
    return 0;
  }

  // *p = count elements of device memory, owned by scope s (release() frees it and nulls *p)
  template <class T>
  int dalloc(Scope s, T **p, size_t count) {
    *p = nullptr;
    if (!count) return 0;
    HIPCHK(hipMalloc((void **)p, count * sizeof(T)));
    owned[s].push_back((void **)p);
    return 0;
  }

  // a dalloc()ed copy of v, queued on the stream
  template <class T>
  int upload(Scope s, T **dst, const std::vector<T> &v) {
    if (int rc = dalloc(s, dst, v.size())) return rc;
    if (!v.empty()) HIPCHK(hipMemcpyAsync(*dst, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, st));
    return 0;
  }

  void release(Scope s) {
    for (void **p : owned[s]) {
      if (*p) (void)hipFree(*p);
      *p = nullptr;
    }
    owned[s].clear();
  }

  // device ms between events a and b, -1 where the phase has not run (timed false) or has no measurement
  double elapsed_ms(int a, int b, bool timed) const {
    float t = 0;
    return timed && hipEventElapsedTime(&t, ev[a], ev[b]) == hipSuccess ? (double)t : -1.0;
  }

 private:
  std::vector<void **> owned[2];
};

inline int no_device_or_null(const char *name) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return fail(SVILS_ERR_DEVICE, "%s: no HIP device available; this library has no CPU path", name);
  return fail(SVILS_ERR_ARG, "%s: null handle", name);
}

// every entry point's first step: a null handle is refused (as "no HIP device" where there is none), else its device is made current
inline int check(const ToolHandle *h, const char *name) {
  if (!h) return no_device_or_null(name);
  HIPCHK(hipSetDevice(h->device));
  return 0;
}

}  // namespace svils_impl
