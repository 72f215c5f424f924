// orbfe_stage.h -- the host plumbing the handles share: the 256-byte alignment rule, the staging block
// (a device buffer, optionally with a pinned twin, carved by a bump offset), the device and stream part
// of a handle with its create / destroy prelude, and three small steps of the batched RANSAC solvers.
// Host only. The layout arithmetic is plain C++ (the per-solver layout functions of the *_core.h files
// and tests/cpp/stage_layout_test.cpp use it without a HIP runtime); what calls HIP is under __HIPCC__.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>

// The one alignment rule of every staged array
inline size_t orbfe_al256(size_t b) { return (b + 255) & ~(size_t)255; }

// A block carved in 256-byte steps. d: the device buffer; h: its pinned twin at the same offsets, if it
// has one. With d == nullptr the block only counts: every address it hands out is null and off ends as the
// bytes the same sequence of takes needs, so one layout function both sizes a buffer and fills it.
struct OrbfeStage {
  uint8_t* d = nullptr;
  uint8_t* h = nullptr;
  size_t cap = 0, off = 0;

  size_t take(size_t bytes) {
    const size_t at = off;
    off += orbfe_al256(bytes);
    return at;
  }
  // reserves count elements; *host receives the host address, the device address is returned
  template <class T>
  T* take(size_t count, T** host) {
    const size_t at = take(sizeof(T) * count);
    if (host) *host = h ? reinterpret_cast<T*>(h + at) : nullptr;
    return d ? reinterpret_cast<T*>(d + at) : nullptr;
  }
  template <class T>
  void take(T*& field, size_t count) {
    field = take<T>(count, nullptr);
  }
  template <class T>
  const T* put(const T* src, size_t count) {
    T* host;
    T* dev = take<T>(count, &host);
    if (count) memcpy(host, src, sizeof(T) * count);
    return dev;
  }
};

// mRansacMaxIts of Sim3Solver (:124-134) and PnPsolver (:155-162): ceil(log(1 - p) / log(1 - epsilon^3))
// with x86's out-of-range conversion, capped by max_iterations and held to >= 1. epsilon comes from each
// solver's own float steps.
inline int ransac_max_its(int n, int min_inliers, float epsilon, double probability, int max_iterations) {
  int n_it;
  if (min_inliers == n) {
    n_it = 1;
  } else {
    const double q = std::ceil(std::log(1 - probability) / std::log(1 - std::pow((double)epsilon, 3.0)));
    n_it = (q > -2147483649.0 && q < 2147483648.0) ? (int)q : INT_MIN;
  }
  return std::max(1, std::min(n_it, max_iterations));
}

// Whether draw i of every iteration's minimal set lies in 0 .. n-1-i (the swap-remove selection's domain)
inline bool ransac_check_draws(const int32_t* rand_idx, int n_hyp, int set_size, int n) {
  for (int k = 0; k < n_hyp; k++)
    for (int i = 0; i < set_size; i++) {
      const int d = rand_idx[(size_t)set_size * k + i];
      if (d < 0 || d > n - 1 - i) return false;
    }
  return true;
}

// count bit masks of src_words words each (packed, from a result buffer) into the caller's rows of
// dst_words >= src_words words; the trailing words of a row are cleared
inline void orbfe_unpack_masks(uint64_t* dst, int dst_words, const uint8_t* src, int src_words, size_t count) {
  for (size_t k = 0; k < count; k++) {
    uint64_t* row = dst + k * (size_t)dst_words;
    memcpy(row, src + 8 * (size_t)src_words * k, 8 * (size_t)src_words);
    for (int w = src_words; w < dst_words; w++) row[w] = 0;
  }
}

#ifdef __HIPCC__
#include <hip/hip_runtime.h>

#include <cstdio>

#include "../../include/orbfe.h"
#include "orbfe_device.h"

// The device and stream part of a handle; device < 0: a host-only handle that never touches HIP
struct OrbfeDev {
  int device = -1;
  hipStream_t stream = nullptr;
};

// After a create's argument checks: the device must exist; makes it current and creates the handle's
// non-blocking stream. fn: the entry point, for the message. On an error the handle's destroy is safe.
inline int orbfe_dev_open(OrbfeDev* dv, int device, const char* fn) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || device >= ndev) {
    char msg[96];
    snprintf(msg, sizeof(msg), "%s: no such HIP device", fn);
    return orbfe_set_error(ORBFE_ERR_HIP, msg);
  }
  dv->device = device;
  hipError_t e = hipSetDevice(device);
  if (e != hipSuccess) return orbfe_set_hip_error(e, "hipSetDevice(device)");
  e = hipStreamCreateWithFlags(&dv->stream, hipStreamNonBlocking);
  if (e != hipSuccess) return orbfe_set_hip_error(e, "hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking)");
  return ORBFE_OK;
}

// The first step of a destroy: makes the device current, waits for the stream and destroys it. Returns
// whether the handle has a device at all, that is, whether there is anything of its to free after this.
inline bool orbfe_dev_close(OrbfeDev* dv) {
  if (dv->device < 0) return false;
  hipSetDevice(dv->device);
  if (dv->stream) {
    hipStreamSynchronize(dv->stream);
    hipStreamDestroy(dv->stream);
    dv->stream = nullptr;
  }
  return true;
}

// In a *_create, after orbfe_dev_open: on a HIP error records it, destroys the half-built handle (which
// frees what it had allocated) and returns the status
#define ORBFE_CREATE_HIP(h, destroy, expr)               \
  do {                                                   \
    hipError_t _e = (expr);                              \
    if (_e != hipSuccess) {                              \
      const int _st = orbfe_set_hip_error(_e, #expr);    \
      destroy(h);                                        \
      return _st;                                        \
    }                                                    \
  } while (0)

inline hipError_t orbfe_stage_alloc(OrbfeStage* s, size_t cap, bool pinned) {
  s->cap = cap;
  hipError_t e = hipMalloc(&s->d, cap);
  if (e == hipSuccess && pinned) e = hipHostMalloc(&s->h, cap, hipHostMallocDefault);
  return e;
}

inline void orbfe_stage_free(OrbfeStage* s) {
  hipFree(s->d);
  if (s->h) hipHostFree(s->h);
  s->d = s->h = nullptr;
}

// [0, off) up, before the launches
inline int orbfe_stage_upload(OrbfeStage* s, hipStream_t stream) {
  if (s->off > 0) ORBFE_HIP_CHECK(hipMemcpyAsync(s->d, s->h, s->off, hipMemcpyHostToDevice, stream));
  return ORBFE_OK;
}

// after the launches: their launch status, [0, off) down, and the wait for the stream
inline int orbfe_stage_download(OrbfeStage* s, hipStream_t stream) {
  ORBFE_HIP_CHECK(hipGetLastError());
  if (s->off > 0) ORBFE_HIP_CHECK(hipMemcpyAsync(s->h, s->d, s->off, hipMemcpyDeviceToHost, stream));
  ORBFE_HIP_CHECK(hipStreamSynchronize(stream));
  return ORBFE_OK;
}
#endif  // __HIPCC__
