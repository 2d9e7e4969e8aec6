// device_res.h — move-only owners of the HIP resources a handle holds (host only, no kernels).
//
// A handle declares its DevStream members first, then its pools, buffers, pinned arrays and events:
// members are destroyed in reverse order, so everything is released while the stream still exists,
// and the handle's destructor is the only place that releases.  A failing acquire sets the error
// text (LOAM_HIP: the HIP call and the line) and returns LOAM_ERR_HIP with the owner left empty;
// a release ignores the HIP status.
#pragma once
#include <algorithm>
#include <atomic>
#include <utility>
#include <vector>

#include "common.h"

namespace loam {

// what the owners hold right now, process-wide (loam_debug_live_resources; defined in core.hip)
enum : int { LIVE_DEVICE = 0, LIVE_PINNED, LIVE_STREAM, LIVE_EVENT, LIVE_KINDS };
extern std::atomic<int64_t> g_live[LIVE_KINDS];

// a non-blocking stream; synchronized before it is destroyed
struct DevStream {
  hipStream_t s = nullptr;
  DevStream() = default;
  DevStream(DevStream&& o) noexcept : s(std::exchange(o.s, nullptr)) {}
  DevStream& operator=(DevStream&& o) noexcept { return std::swap(s, o.s), *this; }
  ~DevStream() {
    if (!s) return;
    (void)hipStreamSynchronize(s);
    (void)hipStreamDestroy(s);
    --g_live[LIVE_STREAM];
  }
  int32_t create() {
    hipStream_t t = nullptr;
    LOAM_HIP(hipStreamCreateWithFlags(&t, hipStreamNonBlocking));
    *this = DevStream{};
    s = t;
    ++g_live[LIVE_STREAM];
    return LOAM_OK;
  }
  operator hipStream_t() const { return s; }
};

struct DevEvent {
  hipEvent_t e = nullptr;
  DevEvent() = default;
  DevEvent(DevEvent&& o) noexcept : e(std::exchange(o.e, nullptr)) {}
  DevEvent& operator=(DevEvent&& o) noexcept { return std::swap(e, o.e), *this; }
  ~DevEvent() {
    if (!e) return;
    (void)hipEventDestroy(e);
    --g_live[LIVE_EVENT];
  }
  int32_t create(unsigned flags = hipEventDefault) {
    hipEvent_t t = nullptr;
    LOAM_HIP(hipEventCreateWithFlags(&t, flags));
    *this = DevEvent{};
    e = t;
    ++g_live[LIVE_EVENT];
    return LOAM_OK;
  }
  operator hipEvent_t() const { return e; }
};

// the fixed, zero-filled device buffers of a handle: allocated at create, freed together
struct DevPool {
  std::vector<void*> ptrs;
  DevPool() = default;
  DevPool(DevPool&& o) noexcept : ptrs(std::move(o.ptrs)) { o.ptrs.clear(); }
  DevPool& operator=(DevPool&& o) noexcept { return ptrs.swap(o.ptrs), *this; }
  ~DevPool() {
    for (void* p : ptrs) (void)hipFree(p);
    g_live[LIVE_DEVICE] -= (int64_t)ptrs.size();
  }
  template <class T>
  int32_t alloc(T** p, size_t count, hipStream_t st) {
    void* q = nullptr;
    const size_t bytes = std::max<size_t>(count, 1) * sizeof(T);
    LOAM_HIP(hipMalloc(&q, bytes));
    ptrs.push_back(q);
    ++g_live[LIVE_DEVICE];
    // zero on the handle's own (non-blocking) stream: a null-stream memset is not ordered
    // before this stream's kernels; create() synchronizes the stream before returning
    LOAM_HIP(hipMemsetAsync(q, 0, bytes, st));
    *p = static_cast<T*>(q);
    return LOAM_OK;
  }
};

// one device buffer grown on demand: reserve() past the capacity frees, then allocates (the old
// contents are gone, the new ones undefined)
template <class T>
struct DevBuf {
  T* p = nullptr;
  size_t cap = 0;
  DevBuf() = default;
  DevBuf(DevBuf&& o) noexcept : p(std::exchange(o.p, nullptr)), cap(std::exchange(o.cap, 0)) {}
  DevBuf& operator=(DevBuf&& o) noexcept { return std::swap(p, o.p), std::swap(cap, o.cap), *this; }
  ~DevBuf() { release(); }
  void release() {
    if (!p) return;
    (void)hipFree(p);
    --g_live[LIVE_DEVICE];
    p = nullptr;
    cap = 0;
  }
  // takes over q (of count elements) from hipMalloc or one of its variants
  void adopt(T* q, size_t count) {
    release();
    if (!q) return;
    p = q;
    cap = count;
    ++g_live[LIVE_DEVICE];
  }
  int32_t reserve(size_t count) {
    count = std::max<size_t>(count, 1);
    if (p && count <= cap) return LOAM_OK;
    release();
    void* q = nullptr;
    LOAM_HIP(hipMalloc(&q, sizeof(T) * count));
    adopt(static_cast<T*>(q), count);
    return LOAM_OK;
  }
  // reserve() and a synchronous zero fill (for work on the null stream)
  int32_t reserve_zeroed(size_t count) {
    TRY(reserve(count));
    LOAM_HIP(hipMemset(p, 0, sizeof(T) * std::max<size_t>(count, 1)));
    return LOAM_OK;
  }
  operator T*() const { return p; }
};

// page-locked host array (hipHostMalloc) with the few vector operations used here
template <typename T>
struct PinnedArray {
  T* p = nullptr;
  size_t n = 0;
  PinnedArray() = default;
  PinnedArray(PinnedArray&& o) noexcept : p(std::exchange(o.p, nullptr)), n(std::exchange(o.n, 0)) {}
  PinnedArray& operator=(PinnedArray&& o) noexcept { return std::swap(p, o.p), std::swap(n, o.n), *this; }
  ~PinnedArray() { release(); }
  void release() {
    if (!p) return;
    (void)hipHostFree(p);
    --g_live[LIVE_PINNED];
    p = nullptr;
    n = 0;
  }
  int32_t assign(size_t count, const T& v, unsigned flags = hipHostMallocDefault) {
    release();
    void* q = nullptr;
    LOAM_HIP(hipHostMalloc(&q, sizeof(T) * std::max<size_t>(count, 1), flags));
    p = static_cast<T*>(q);
    n = count;
    ++g_live[LIVE_PINNED];
    for (size_t i = 0; i < n; ++i) p[i] = v;
    return LOAM_OK;
  }
  // mapped and coherent, for the device to read or write in place: *dev is its device address
  template <class U>
  int32_t assign_mapped(size_t count, const T& v, U** dev) {
    void* dp = nullptr;
    TRY(assign(count, v, hipHostMallocMapped | hipHostMallocCoherent));
    LOAM_HIP(hipHostGetDevicePointer(&dp, p, 0));
    *dev = static_cast<T*>(dp);
    return LOAM_OK;
  }
  T& operator[](size_t i) { return p[i]; }
  const T& operator[](size_t i) const { return p[i]; }
  T* data() { return p; }
  size_t size() const { return n; }
};

}  // namespace loam
