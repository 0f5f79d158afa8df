// colate_amd/csrc/condcoal_device.hpp -- what the two device walkers of `Colate --mode CondCoalRates` share
// (condcoal_kernel.hip: one table; condcoal_pairs_kernel.hip: --pairs), and nothing else includes: the launch constants,
// the slab row, the prefix scan over a tree's DFS leaf order, and CcDeviceWalker: the device, the run's constants on it
// and the two slots through which chunks of trees are staged.  The kernels and what becomes of their results are each
// walker's own.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "colate_amd.h"
#include "colate_internal.h"
#include "condcoal.h"
#include "condcoal_walk.hpp"

namespace colate_cc {

constexpr int kBlock = 256;  // lanes per workgroup = walks per batch = rows of a slab
constexpr int kMaxGrid = 1024;

struct SlabRow {
  double* p;  // this lane's column of the slab: slot c at p[c * kBlock]
  __device__ void add(int c, double v) { p[(size_t)c * kBlock] += v; }
};

// Workgroups for `work` units of a walk kernel: the slabs take kBlock * S doubles per workgroup, at most ~2 GiB of them.
inline int slab_grid(size_t work, int S) {
  const size_t slab_bytes = (size_t)kBlock * S * sizeof(double);
  return (int)std::max<size_t>(1, std::min<size_t>({(size_t)kMaxGrid, work, ((size_t)2 << 30) / slab_bytes}));
}

// The prefix counts of one tree, by the whole workgroup: pre[row][q] = the leaves x among the first q of the DFS leaf
// order for which counts(row, x), pre[row][N] their number.  Row by row: per-lane chunk counts, a serial scan of the kBlock
// partials, per-lane running sums.  [q0, q1): the calling lane's positions, ceil(N / kBlock) from tid times that, which a
// kernel works out once for all its trees.  The rows are written when it returns (the block is synchronised, not fenced).
template <class Counts>
__device__ __forceinline__ void cc_prefix_rows(int N, int q0, int q1, int rows, const int* leaf, int* pre, Counts counts) {
  __shared__ int s_part[kBlock];
  const int tid = threadIdx.x;
  for (int row = 0; row < rows; row++) {
    int cnt = 0;
    for (int q = q0; q < q1; q++) cnt += counts(row, leaf[q]);
    s_part[tid] = cnt;
    __syncthreads();
    if (tid == 0) {
      int run = 0;
      for (int i = 0; i < kBlock; i++) {
        const int c = s_part[i];
        s_part[i] = run;
        run += c;
      }
      pre[row * (N + 1) + N] = run;
    }
    __syncthreads();
    int run = s_part[tid];
    for (int q = q0; q < q1; q++) {
      pre[row * (N + 1) + q] = run;
      run += counts(row, leaf[q]);
    }
    __syncthreads();
  }
}

// inside a member of a CcWalker
#define CC_TRY(expr)                                                                                      \
  do {                                                                                                    \
    hipError_t e_ = (expr);                                                                               \
    if (e_ != hipSuccess) return fail(std::string(#expr) + ": " + hipGetErrorString(e_), COLATE_EHIP);    \
  } while (0)

// Device and pinned host memory that goes when its owner goes.
class CcBuffers {
 public:
  CcBuffers() = default;
  CcBuffers(const CcBuffers&) = delete;
  CcBuffers& operator=(const CcBuffers&) = delete;
  ~CcBuffers() {
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

class CcDeviceWalker : public CcWalker {
 public:
  ~CcDeviceWalker() override {
    if (stream_) (void)hipStreamSynchronize(stream_);  // (before buf_ goes)
    for (Slot& s : slot_)
      for (hipEvent_t e : {s.ev0, s.evk, s.ev1})
        if (e) (void)hipEventDestroy(e);
    if (stream_) (void)hipStreamDestroy(stream_);
  }

 protected:
  template <class T>
  struct Staged {  // an array on its way to or from the device: the pinned copy and the device's
    T *h = nullptr, *d = nullptr;
  };
  struct Slot {  // the trees of one launch
    int T = 0;
    Staged<int> parent, lo, hi, leaf, block;
    Staged<double> bl;
    Staged<float> factor;
    hipEvent_t ev0 = nullptr, evk = nullptr, ev1 = nullptr;  // kernels start / kernels end / results copied back
    bool busy = false;
  };

  // Opens the device (-1: the calling thread's), puts group, ages, epochs and efocal there and sh_ over them (is_cond and
  // cond_empty are left to the walker), and makes the two slots for max_trees trees each (`block` only with_blocks).
  bool open(int device, const CcRun& run, int max_trees, bool with_blocks) {
    colate::mark_device_touched();
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return fail("no HIP device", COLATE_EHIP);
    if (device < 0 && hipGetDevice(&device) != hipSuccess) device = 0;
    if (device >= n) return fail("no HIP device " + std::to_string(device), COLATE_EHIP);
    device_ = device;
    N_ = run.N;
    max_trees_ = std::max(1, max_trees);
    CC_TRY(hipSetDevice(device));
    CC_TRY(hipStreamCreateWithFlags(&stream_, hipStreamNonBlocking));
    int* group = nullptr;
    double* ages = nullptr;
    float *epochs = nullptr, *efocal = nullptr;
    if (!upload(group, run.group) || !upload(epochs, run.epochs) || !upload(efocal, run.efocal)) return false;
    if (!run.ages.empty() && !upload(ages, run.ages)) return false;
    sh_.N = run.N;
    sh_.G = run.G;
    sh_.E = run.E();
    sh_.EF = run.EF();
    sh_.group = group;
    sh_.is_cond = nullptr;
    sh_.cond_empty = 0;
    sh_.ages = ages;
    sh_.epochs = epochs;
    sh_.efocal = efocal;
    const size_t T = max_trees_, nn = 2 * (size_t)N_ - 1;
    for (Slot& s : slot_) {
      if (!make(s.parent, T * nn) || !make(s.lo, T * nn) || !make(s.hi, T * nn) || !make(s.leaf, T * N_) || !make(s.bl, T * nn) ||
          !make(s.factor, T) || (with_blocks && !make(s.block, T)))
        return false;
      CC_TRY(hipEventCreate(&s.ev0));
      CC_TRY(hipEventCreate(&s.evk));
      CC_TRY(hipEventCreate(&s.ev1));
    }
    return true;
  }
  template <class T>
  bool upload(T*& dst, const std::vector<T>& v) {
    CC_TRY(buf_.device(dst, v.size()));
    if (!v.empty()) CC_TRY(hipMemcpy(dst, v.data(), sizeof(T) * v.size(), hipMemcpyHostToDevice));
    return true;
  }
  template <class T>
  bool make(Staged<T>& a, size_t n) {
    CC_TRY(buf_.pinned(a.h, n));
    CC_TRY(buf_.device(a.d, n));
    return true;
  }
  // n elements into the pinned copy and, on the stream, on to the device
  template <class T>
  bool send(Staged<T>& a, const T* src, size_t n) {
    std::memcpy(a.h, src, sizeof(T) * n);
    CC_TRY(hipMemcpyAsync(a.d, a.h, sizeof(T) * n, hipMemcpyHostToDevice, stream_));
    return true;
  }

  bool accepts(const CcChunk& c) {
    return (c.T <= max_trees_ && c.N == N_) || fail("condcoal: chunk larger than the device buffers", COLATE_EINVAL);
  }
  // Trees [t0, t1) of the chunk into the slot (which is not busy), their uploads enqueued.
  bool stage(Slot& s, const CcChunk& c, int t0, int t1) {
    const size_t T = t1 - t0, N = N_, nn = 2 * N - 1;
    s.T = (int)T;
    CC_TRY(hipSetDevice(device_));
    return send(s.parent, c.parent.data() + t0 * nn, T * nn) && send(s.lo, c.lo.data() + t0 * nn, T * nn) &&
           send(s.hi, c.hi.data() + t0 * nn, T * nn) && send(s.leaf, c.leaf.data() + t0 * N, T * N) &&
           send(s.bl, c.bl.data() + t0 * nn, T * nn) && send(s.factor, c.factor.data() + t0, T) &&
           (!s.block.h || send(s.block, c.block.data() + t0, T));
  }
  // Waits until a busy slot's results are on the host (ev1) and books its kernel time.
  bool wait(Slot& s) {
    CC_TRY(hipEventSynchronize(s.ev1));
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, s.ev0, s.evk) == hipSuccess) gpu_s_ += ms * 1e-3;
    return true;
  }

  int device_ = 0, N_ = 0, max_trees_ = 0;
  CcShared sh_{};
  CcBuffers buf_;
  hipStream_t stream_ = nullptr;
  Slot slot_[2];
  int cur_ = 0;  // the slot of the next launch
};

}  // namespace colate_cc
