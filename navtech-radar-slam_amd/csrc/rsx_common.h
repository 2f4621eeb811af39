// rsx_common.h -- shared host-side plumbing of librsx.so (error reporting, HIP checks, owning HIP resources).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <new>
#include <stdexcept>
#include <string>
#include <utility>

#include "rsx.h"
#include "rsx_diag.h"

namespace rsx {

std::string &last_error();

inline int fail(int code, const char *fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  last_error() = buf;
  return code;
}

// Experiment / tuning knobs read from the environment exist only in -DRSX_EXPERIMENTS builds (make EXPERIMENTS=1, what
// tools/prof*.sh and tools/spectral/* build): the product library has no hidden switches.  The experiments build carries
// tuning numbers and profiling of the kernels the product runs, not alternative kernels: a variant that lost its A/B test
// is deleted (its measurement stays in DESIGN.md, its code in git history).
inline const char *exp_env(const char *name) {
#ifdef RSX_EXPERIMENTS
  return std::getenv(name);
#else
  (void)name;
  return nullptr;
#endif
}

// Exception firewall of the C-ABI ("no C++ exceptions cross the ABI"; the reference lets nanoflann's
// std::runtime_error escape, NF.hpp:1228,1324).  EVERY extern "C" entry that returns a status is a function-try-block
//     int rsx_xxx(...) try { ... } RSX_CATCH_ALL
// so a std::bad_alloc from a host container (std::vector growth, new), a std::system_error from a mutex or anything else
// thrown below comes back as a status with rsx_last_error_string() set.
inline int on_exception() noexcept {
  int code = RSX_ERR_INTERNAL;
  try {
    try {
      throw;
    } catch (const std::bad_alloc &) {
      code = RSX_ERR_OOM;
      return fail(code, "host allocation failed (std::bad_alloc)");
    } catch (const std::length_error &e) {
      code = RSX_ERR_OOM;
      return fail(code, "host allocation failed (%s)", e.what());
    } catch (const std::exception &e) {
      return fail(code, "unexpected exception: %s", e.what());
    } catch (...) {
      return fail(code, "unexpected exception");
    }
  } catch (...) {  // (recording the message itself failed)
    return code;
  }
}
#define RSX_CATCH_ALL \
  catch (...) {       \
    return rsx::on_exception(); \
  }

#define RSX_HIP(expr)                                                                         \
  do {                                                                                        \
    hipError_t _e = (expr);                                                                   \
    if (_e != hipSuccess)                                                                     \
      return rsx::fail(_e == hipErrorOutOfMemory ? RSX_ERR_OOM : RSX_ERR_HIP, "%s failed: %s", \
                       #expr, hipGetErrorString(_e));                                         \
  } while (0)

#define RSX_TRY(expr)          \
  do {                         \
    int _s = (expr);           \
    if (_s != RSX_OK) return _s; \
  } while (0)

// the device checks every rsx_*_create starts with
inline int check_device(int device) {
  const int ndev = rsx_device_count();
  if (ndev <= 0) return fail(RSX_ERR_NO_DEVICE, "no HIP device visible (librsx has no CPU fallback)");
  if (device < 0 || device >= ndev) return fail(RSX_ERR_NO_DEVICE, "device %d out of range (%d visible)", device, ndev);
  return RSX_OK;
}

// Owning HIP resources (DevBuf, PinnedBuf, Stream, Event): each frees what it holds when it goes, so a handle's destroy is
// "synchronise its streams, delete".  Move-only; moving swaps, so what the target held goes with the source.

// growable device buffer (never shrinks); contents preserved on growth when keep=true
struct DevBuf {
  void *p = nullptr;
  size_t bytes = 0;
  DevBuf() = default;
  DevBuf(DevBuf &&o) noexcept { *this = std::move(o); }
  DevBuf &operator=(DevBuf &&o) noexcept {
    std::swap(p, o.p);
    std::swap(bytes, o.bytes);
    return *this;
  }
  ~DevBuf() {
    if (p) (void)hipFree(p);
  }
  int reserve(size_t want, hipStream_t s, bool keep) {
    if (want <= bytes) return RSX_OK;
    size_t nb = bytes ? bytes : 4096;
    while (nb < want) nb *= 2;
    void *np = nullptr;
    RSX_HIP(hipMalloc(&np, nb));
    if (keep && p && bytes) {
      hipError_t e = hipMemcpyAsync(np, p, bytes, hipMemcpyDeviceToDevice, s);
      if (e == hipSuccess) e = hipStreamSynchronize(s);
      if (e != hipSuccess) {
        (void)hipFree(np);
        return fail(RSX_ERR_HIP, "DevBuf grow copy: %s", hipGetErrorString(e));
      }
    } else if (p) {
      hipError_t e = hipStreamSynchronize(s);
      if (e != hipSuccess) {
        (void)hipFree(np);
        return fail(RSX_ERR_HIP, "DevBuf grow sync: %s", hipGetErrorString(e));
      }
    }
    if (p) (void)hipFree(p);
    p = np;
    bytes = nb;
    return RSX_OK;
  }
  template <typename T>
  T *as() const {
    return static_cast<T *>(p);
  }
};

// pinned host buffer; reserve(want) frees and allocates exactly `want` bytes when it holds fewer (contents not kept: the
// caller picks the size policy)
struct PinnedBuf {
  void *p = nullptr;
  size_t bytes = 0;
  PinnedBuf() = default;
  PinnedBuf(PinnedBuf &&o) noexcept { *this = std::move(o); }
  PinnedBuf &operator=(PinnedBuf &&o) noexcept {
    std::swap(p, o.p);
    std::swap(bytes, o.bytes);
    return *this;
  }
  ~PinnedBuf() {
    if (p) (void)hipHostFree(p);
  }
  int reserve(size_t want) {
    if (want <= bytes) return RSX_OK;
    if (p) (void)hipHostFree(p);
    p = nullptr;
    bytes = 0;
    RSX_HIP(hipHostMalloc(&p, want, hipHostMallocDefault));
    bytes = want;
    return RSX_OK;
  }
};

// non-blocking stream; null until create()
struct Stream {
  hipStream_t s = nullptr;
  Stream() = default;
  Stream(Stream &&o) noexcept { *this = std::move(o); }
  Stream &operator=(Stream &&o) noexcept {
    std::swap(s, o.s);
    return *this;
  }
  ~Stream() {
    if (s) (void)hipStreamDestroy(s);
  }
  hipError_t create() { return hipStreamCreateWithFlags(&s, hipStreamNonBlocking); }
  operator hipStream_t() const { return s; }
};

// event without timing (timing = true: with, for hipEventElapsedTime); null until create()
struct Event {
  hipEvent_t e = nullptr;
  Event() = default;
  Event(Event &&o) noexcept { *this = std::move(o); }
  Event &operator=(Event &&o) noexcept {
    std::swap(e, o.e);
    return *this;
  }
  ~Event() {
    if (e) (void)hipEventDestroy(e);
  }
  hipError_t create(bool timing = false) { return timing ? hipEventCreate(&e) : hipEventCreateWithFlags(&e, hipEventDisableTiming); }
  operator hipEvent_t() const { return e; }
};

// a handle whose workspaces are shared by every call: a call on another stream than the previous one is ordered behind it
struct StreamOrder {
  hipStream_t last = nullptr;
  Event switched;
  int enter(hipStream_t s) {
    if (last && last != s) {
      if (!switched) RSX_HIP(switched.create());
      // (a previous stream the caller has destroyed in the meantime has drained: nothing to wait for)
      if (hipEventRecord(switched, last) == hipSuccess) RSX_HIP(hipStreamWaitEvent(s, switched, 0));
      else (void)hipGetLastError();
    }
    last = s;
    return RSX_OK;
  }
};

// a librsx handle owned by another one, freed by its own rsx_*_destroy: Owned<rsx_icp, rsx_icp_destroy>
template <auto Destroy>
struct Destroyer {
  template <typename T>
  void operator()(T *h) const {
    (void)Destroy(h);
  }
};
template <typename T, auto Destroy>
using Owned = std::unique_ptr<T, Destroyer<Destroy>>;

}  // namespace rsx
