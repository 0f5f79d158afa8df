// colate_amd/csrc/condcoal_device.hpp -- what the two device walkers of `Colate --mode CondCoalRates` share
// (condcoal_kernel.hip: one table; condcoal_pairs_kernel.hip: --pairs), and nothing else includes: the launch constants,
// the slab row, the prefix scan over a tree's DFS leaf order, and CcDeviceWalker: on device_stage.hpp's opened device
// and staged arrays, the run's constants and the two slots through which chunks of trees are staged.  The kernels and
// what becomes of their results are each walker's own.
#pragma once
#include "condcoal.h"
#include "condcoal_walk.hpp"
#include "device_stage.hpp"

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

using colate::Staged;

class CcDeviceWalker : public colate::DeviceStage<CcWalker> {
 protected:
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
    if (!open_device(device)) return false;
    N_ = run.N;
    max_trees_ = std::max(1, max_trees);
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
      if (!make_event(s.ev0) || !make_event(s.evk) || !make_event(s.ev1)) return false;
    }
    return true;
  }
  bool accepts(const CcChunk& c) {
    return (c.T <= max_trees_ && c.N == N_) || fail("condcoal: chunk larger than the device buffers", COLATE_EINVAL);
  }
  // Trees [t0, t1) of the chunk into the slot (which is not busy), their uploads enqueued.
  bool stage(Slot& s, const CcChunk& c, int t0, int t1) {
    const size_t T = t1 - t0, N = N_, nn = 2 * N - 1;
    s.T = (int)T;
    WALKER_TRY(hipSetDevice(device_));
    return send(s.parent, c.parent.data() + t0 * nn, T * nn) && send(s.lo, c.lo.data() + t0 * nn, T * nn) &&
           send(s.hi, c.hi.data() + t0 * nn, T * nn) && send(s.leaf, c.leaf.data() + t0 * N, T * N) &&
           send(s.bl, c.bl.data() + t0 * nn, T * nn) && send(s.factor, c.factor.data() + t0, T) &&
           (!s.block.h || send(s.block, c.block.data() + t0, T));
  }
  // Waits until a busy slot's results are on the host (ev1), books its kernel time and frees the slot.
  bool wait(Slot& s) {
    if (!wait_event(s.ev1, s.ev0, s.evk)) return false;
    s.busy = false;
    return true;
  }

  int N_ = 0, max_trees_ = 0;
  CcShared sh_{};
  Slot slot_[2];
  int cur_ = 0;  // the slot of the next launch
};

}  // namespace colate_cc
