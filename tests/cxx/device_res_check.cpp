// The resource owners of csrc/device_res.h, stand-alone (tests/test_device_res.py builds and runs it).
//   device_res_check 0   no device: every acquire fails with LOAM_ERR_HIP and a text naming the HIP
//                        call, leaves its owner empty and the live counts unchanged; destroying an
//                        empty or moved-from owner does nothing
//   device_res_check 1   a device: acquire, use, grow, release; the live counts return to their start
#include <array>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "device_res.h"

using namespace loam;
using Live = std::array<int64_t, 4>;

static int failures = 0;
#define CHECK(cond)                                                  \
  do {                                                               \
    if (!(cond)) {                                                   \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      ++failures;                                                    \
    }                                                                \
  } while (0)

static Live live() {
  Live v{};
  CHECK(loam_debug_live_resources(v.data()) == LOAM_OK);
  return v;
}

// rc is LOAM_ERR_HIP, the error text names the HIP call, the counts did not move
static void check_failed(int32_t rc, const char* hip_call, const Live& before) {
  CHECK(rc == LOAM_ERR_HIP);
  const std::string msg = loam_last_error();
  CHECK(!msg.empty());
  if (msg.find(hip_call) == std::string::npos) {
    std::printf("FAILED: \"%s\" does not name %s\n", msg.c_str(), hip_call);
    ++failures;
  }
  CHECK(live() == before);
  set_error("");
}

static int no_device() {
  const Live start = live();
  {
    DevStream s;
    check_failed(s.create(), "hipStreamCreateWithFlags", start);
    CHECK(s.s == nullptr);
    DevStream moved(std::move(s));
    CHECK(moved.s == nullptr && s.s == nullptr);
  }
  {
    DevEvent e;
    check_failed(e.create(), "hipEventCreateWithFlags", start);
    check_failed(e.create(hipEventDisableTiming), "hipEventCreateWithFlags", start);
    CHECK(e.e == nullptr);
    DevEvent moved(std::move(e));
    CHECK(moved.e == nullptr && e.e == nullptr);
  }
  {
    DevPool pool;
    int* p = nullptr;
    check_failed(pool.alloc(&p, 1000, nullptr), "hipMalloc", start);
    CHECK(p == nullptr && pool.ptrs.empty());
    DevPool moved(std::move(pool));
    CHECK(moved.ptrs.empty() && pool.ptrs.empty());
  }
  {
    DevBuf<float> b;
    check_failed(b.reserve(8), "hipMalloc", start);
    CHECK(b.p == nullptr && b.cap == 0);
    check_failed(b.reserve(300), "hipMalloc", start);  // a second reserve after a failed one
    check_failed(b.reserve_zeroed(8), "hipMalloc", start);
    CHECK(b.p == nullptr && b.cap == 0);
    DevBuf<float> moved(std::move(b));
    CHECK(moved.p == nullptr && b.p == nullptr);
  }
  {
    PinnedArray<double> a;
    double* dev = nullptr;
    check_failed(a.assign(16, 1.0), "hipHostMalloc", start);
    check_failed(a.assign_mapped(16, 1.0, &dev), "hipHostMalloc", start);
    CHECK(a.data() == nullptr && a.size() == 0 && dev == nullptr);
    PinnedArray<double> moved(std::move(a));
    CHECK(moved.data() == nullptr && a.data() == nullptr);
  }
  CHECK(live() == start);
  return failures;
}

static int with_device() {
  if (hipSetDevice(0) != hipSuccess) return std::printf("FAILED: hipSetDevice\n"), 1;
  const Live start = live();
  {
    DevStream st;
    CHECK(st.create() == LOAM_OK && st.s != nullptr);
    DevEvent ev;
    CHECK(ev.create() == LOAM_OK && ev.e != nullptr);
    CHECK(live()[LIVE_STREAM] == start[LIVE_STREAM] + 1 && live()[LIVE_EVENT] == start[LIVE_EVENT] + 1);

    DevPool pool;
    int* d = nullptr;
    CHECK(pool.alloc(&d, 1000, st) == LOAM_OK && d != nullptr);
    std::vector<int> back(1000, -1);
    CHECK(hipMemcpyAsync(back.data(), d, sizeof(int) * 1000, hipMemcpyDeviceToHost, st) == hipSuccess);
    CHECK(hipStreamSynchronize(st) == hipSuccess);
    CHECK(back == std::vector<int>(1000, 0));
    CHECK(live()[LIVE_DEVICE] == start[LIVE_DEVICE] + 1);

    const int64_t held = live()[LIVE_DEVICE];
    DevBuf<float> b;
    for (size_t n : {8, 300, 8}) CHECK(b.reserve(n) == LOAM_OK && b.p != nullptr && b.cap >= n);
    CHECK(live()[LIVE_DEVICE] == held + 1);
    DevBuf<float> moved(std::move(b));
    CHECK(b.p == nullptr && moved.p != nullptr && live()[LIVE_DEVICE] == held + 1);

    PinnedArray<double> a;
    double* dev = nullptr;
    CHECK(a.assign(16, 1.5) == LOAM_OK && a.size() == 16 && a[15] == 1.5);
    CHECK(a.assign_mapped(32, 2.5, &dev) == LOAM_OK && a.size() == 32 && a[31] == 2.5 && dev != nullptr);
    CHECK(live()[LIVE_PINNED] == start[LIVE_PINNED] + 1);
  }
  CHECK(live() == start);
  return failures;
}

int main(int argc, char** argv) {
  const bool device = argc > 1 && std::strcmp(argv[1], "1") == 0;
  const int bad = device ? with_device() : no_device();
  std::printf("%s: %d failure(s)\n", device ? "device" : "no device", bad);
  return bad ? 1 : 0;
}
