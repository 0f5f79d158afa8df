// colate_amd/csrc/device_stage.hpp -- what every device walker of the tree-based estimators owns, whatever it walks
// (condcoal_device.hpp: CondCoalRates; coalrate_device.hpp: the two CoalRate modes): the opened device, one stream, its
// events, device and pinned memory that goes with the walker, and arrays staged through a pinned copy.  Nothing here
// knows about trees: the table fill's DeviceFill (fill_kernel.hip), which runs several streams of its own, takes
// DeviceBuffers and WALKER_TRY from here.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "colate_amd.h"
#include "colate_internal.h"

namespace colate {

// inside a member of a walker (a class with fail(what, code))
#define WALKER_TRY(expr)                                                                                     \
  do {                                                                                                       \
    hipError_t e_ = (expr);                                                                                  \
    if (e_ != hipSuccess) return this->fail(std::string(#expr) + ": " + hipGetErrorString(e_), COLATE_EHIP); \
  } while (0)

// Device and pinned host memory that goes when its owner goes.
class DeviceBuffers {
 public:
  DeviceBuffers() = default;
  DeviceBuffers(const DeviceBuffers&) = delete;
  DeviceBuffers& operator=(const DeviceBuffers&) = delete;
  ~DeviceBuffers() {
    for (void* h : pinned_) (void)hipHostFree(h);
    for (void* d : device_) (void)hipFree(d);
  }
  template <class T>
  hipError_t device(T*& p, size_t n) {
    const hipError_t e = hipMalloc((void**)&p, sizeof(T) * std::max<size_t>(1, n));
    if (e == hipSuccess) device_.push_back(p);
    return e;
  }
  template <class T>
  hipError_t pinned(T*& p, size_t n) {
    const hipError_t e = hipHostMalloc((void**)&p, sizeof(T) * std::max<size_t>(1, n), hipHostMallocDefault);
    if (e == hipSuccess) pinned_.push_back(p);
    return e;
  }

 private:
  std::vector<void*> device_, pinned_;
};

template <class T>
struct Staged {  // an array on its way to or from the device: the pinned copy and the device's
  T *h = nullptr, *d = nullptr;
};

// Walker: an interface with fail(what, code) and gpu_s_ (colate_cc::CcWalker, colate_cr::BlockSumWalker).
template <class Walker>
class DeviceStage : public Walker {
 public:
  ~DeviceStage() override {
    if (stream_) (void)hipStreamSynchronize(stream_);  // (before buf_ goes)
    for (hipEvent_t e : events_) (void)hipEventDestroy(e);
    if (stream_) (void)hipStreamDestroy(stream_);
  }

 protected:
  // Opens the device (-1: the calling thread's) and makes the stream.
  bool open_device(int device) {
    mark_device_touched();
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return this->fail("no HIP device", COLATE_EHIP);
    if (device < 0 && hipGetDevice(&device) != hipSuccess) device = 0;
    if (device >= n) return this->fail("no HIP device " + std::to_string(device), COLATE_EHIP);
    device_ = device;
    WALKER_TRY(hipSetDevice(device));
    WALKER_TRY(hipStreamCreateWithFlags(&stream_, hipStreamNonBlocking));
    return true;
  }
  bool make_event(hipEvent_t& e) {
    WALKER_TRY(hipEventCreate(&e));
    events_.push_back(e);
    return true;
  }
  template <class T>
  bool upload(T*& dst, const std::vector<T>& v) {
    WALKER_TRY(buf_.device(dst, v.size()));
    if (!v.empty()) WALKER_TRY(hipMemcpy(dst, v.data(), sizeof(T) * v.size(), hipMemcpyHostToDevice));
    return true;
  }
  template <class T>
  bool make(Staged<T>& a, size_t n) {
    WALKER_TRY(buf_.pinned(a.h, n));
    WALKER_TRY(buf_.device(a.d, n));
    return true;
  }
  // n elements into the pinned copy and, on the stream, on to the device
  template <class T>
  bool send(Staged<T>& a, const T* src, size_t n) {
    std::memcpy(a.h, src, sizeof(T) * n);
    WALKER_TRY(hipMemcpyAsync(a.d, a.h, sizeof(T) * n, hipMemcpyHostToDevice, stream_));
    return true;
  }
  // Waits for `done` and books the kernel time between two events recorded before it.
  bool wait_event(hipEvent_t done, hipEvent_t from, hipEvent_t to) {
    WALKER_TRY(hipEventSynchronize(done));
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, from, to) == hipSuccess) this->gpu_s_ += ms * 1e-3;
    return true;
  }

  int device_ = 0;
  DeviceBuffers buf_;
  hipStream_t stream_ = nullptr;

 private:
  std::vector<hipEvent_t> events_;
};

}  // namespace colate
