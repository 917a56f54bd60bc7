// svils_tool.h -- the scaffold of the standalone device handles: one device, one stream, a set of events that only
// grows, and device buffers tracked in two scopes -- the handle's lifetime and the current graph's.  A scope owns each
// buffer once, with the element count it was allocated for; a buffer that has to grow is replaced through reserve().
//
//   svils_findk.hip   -findk: label propagation over a top-5 sparse gamma
//   svils_lc.hip      -gml / -lcstats: the link communities of a fitted model
//   svils_batch.hip   -batch-gpu / -rnode / -rpair / -infset: the exact model over all pairs, sampled pairs, stars
//   svils_orig.hip    -orig: the full K x K blockmodel (svils_orig.h)
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

  // at least nev events (a graph whose sweep takes more launches than the last one's)
  int need_events(size_t nev) {
    while (ev.size() < nev) {
      hipEvent_t e = nullptr;
      HIPCHK(hipEventCreate(&e));
      ev.push_back(e);
    }
    return 0;
  }

  // *p = count elements of device memory, owned by scope s (release() frees it and nulls *p).  *p must not be owned already.
  template <class T>
  int dalloc(Scope s, T **p, size_t count) {
    *p = nullptr;
    if (!count) return 0;
    HIPCHK(hipMalloc((void **)p, count * sizeof(T)));
    owned[s].push_back({(void **)p, count});
    return 0;
  }

  // the elements scope s holds for *p: 0 if it holds none (never allocated, or released with the scope)
  template <class T>
  size_t capacity(Scope s, T *const *p) const {
    for (const Owned &o : owned[s])
      if (o.p == (void **)p) return o.count;
    return 0;
  }

  // *p, owned by scope s, holds at least `need` elements: kept while it suffices, otherwise the stream is waited for (work
  // in flight may still use the old buffer), the old buffer is freed and its entry dropped, and a new one is dalloc()ed --
  // the scope lists *p once however often it grows.  The contents are not kept.
  template <class T>
  int reserve(Scope s, T **p, size_t need) {
    if (need <= capacity(s, p)) return 0;
    for (size_t i = 0; i < owned[s].size(); ++i)
      if (owned[s][i].p == (void **)p) {
        HIPCHK(hipStreamSynchronize(st));
        (void)hipFree(*p);
        *p = nullptr;
        owned[s].erase(owned[s].begin() + i);
        break;
      }
    return dalloc(s, p, need);
  }

  // a dalloc()ed copy of v, queued on the stream
  template <class T>
  int upload(Scope s, T **dst, const std::vector<T> &v) {
    if (int rc = dalloc(s, dst, v.size())) return rc;
    if (!v.empty()) HIPCHK(hipMemcpyAsync(*dst, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, st));
    return 0;
  }

  void release(Scope s) {
    for (const Owned &o : owned[s]) {
      if (*o.p) (void)hipFree(*o.p);
      *o.p = nullptr;
    }
    owned[s].clear();
  }

  // device ms between events a and b, -1 where the phase has not run (timed false) or has no measurement
  double elapsed_ms(int a, int b, bool timed) const {
    float t = 0;
    return timed && hipEventElapsedTime(&t, ev[a], ev[b]) == hipSuccess ? (double)t : -1.0;
  }
  // the sum over nlaunch launches of the brackets ev[first + 2 b] .. ev[first + 1 + 2 b], -1 where the sweep has not run
  double launches_ms(int first, uint32_t nlaunch, bool timed) const {
    if (!timed) return -1.0;
    double ms = 0.0;
    for (uint32_t b = 0; b < nlaunch; ++b) ms += elapsed_ms(first + 2 * (int)b, first + 1 + 2 * (int)b, true);
    return ms;
  }

 private:
  struct Owned {
    void **p;       // the handle's pointer
    size_t count;   // elements allocated for it
  };
  std::vector<Owned> owned[2];
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
