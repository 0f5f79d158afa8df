// colate_amd/csrc/coalrate_device.hpp -- what the device walkers of the two CoalRate modes share (coalrate_kernel.hip:
// local_ancestry; coalrate_tree_kernel.hip: tree), and nothing else includes: on device_stage.hpp's opened device, the two
// slots through which chunks of calls are staged, the calls-per-workgroup rule of the first kernel, and the per-block sums
// [block][cells] that stay on the device until finish().  A mode's walker adds its LDS sizing, its staged arrays and its
// two kernel launches.
#pragma once
#include "coalrate.h"
#include "device_stage.hpp"

namespace colate_cr {

using colate::Staged;

constexpr int kMaxLanes = 256;            // lanes per workgroup
constexpr size_t kLdsBytes = 160 * 1024;  // the LDS of a CU, which one workgroup may have whole (the launch opts in)
constexpr int kWavesPerCu = 8;            // resident waves per CU beyond which packing calls into a workgroup pays

// Chunk: N, T and block[T] beside the mode's arrays.  Arrays: the Staged arrays of one slot.
template <class Chunk, class Arrays>
class BlockSumDeviceWalker : public colate::DeviceStage<BlockSumWalker<Chunk>> {
 public:
  ~BlockSumDeviceWalker() override {
    if (this->stream_) (void)hipStreamSynchronize(this->stream_);  // (before the sums go)
    if (num_) (void)hipFree(num_);
    if (den_) (void)hipFree(den_);
  }

  bool submit(const Chunk& c) final {
    if (c.T == 0) return true;
    if (c.N != N_) return this->fail(std::string(name_) + ": chunk of another N", COLATE_EINVAL);
    WALKER_TRY(hipSetDevice(this->device_));
    int max_block = 0;
    for (int k = 0; k < c.T; k++) max_block = std::max(max_block, c.block[k]);
    if (!grow(max_block + 1)) return false;
    for (int t0 = 0; t0 < c.T; t0 += max_calls_) {
      const int T = std::min(c.T - t0, max_calls_);
      Slot& s = slot_[cur_];
      cur_ ^= 1;
      if (s.busy && !wait(s)) return false;
      if (!stage(s, c, t0, T)) return false;
      WALKER_TRY(hipEventRecord(s.ev0, this->stream_));
      if (!launch(s, T)) return false;
      WALKER_TRY(hipEventRecord(s.ev1, this->stream_));
      s.busy = true;
    }
    return true;
  }

  bool finish(CrSums& out) final {
    WALKER_TRY(hipSetDevice(this->device_));
    for (Slot& s : slot_)
      if (s.busy && !wait(s)) return false;
    WALKER_TRY(hipStreamSynchronize(this->stream_));
    const size_t n = (size_t)blocks_ * cells_;
    out.blocks = blocks_;
    out.num.assign(n, 0.0);
    out.den.assign(n, 0.0);
    if (n) {
      WALKER_TRY(hipMemcpy(out.num.data(), num_, sizeof(double) * n, hipMemcpyDeviceToHost));
      WALKER_TRY(hipMemcpy(out.den.data(), den_, sizeof(double) * n, hipMemcpyDeviceToHost));
    }
    return true;
  }

 protected:
  struct Slot : Arrays {
    hipEvent_t ev0 = nullptr, ev1 = nullptr;  // kernels start / kernels end
    bool busy = false;
  };
  struct Shape {
    int cpw, lanes, grid;  // calls per workgroup, lanes per workgroup, workgroups
  };

  explicit BlockSumDeviceWalker(const char* name) : name_(name) {}
  // Calls [t0, t0 + T) of the chunk into the slot, their uploads enqueued; then the two kernels over them.
  virtual bool stage(Slot& s, const Chunk& c, int t0, int T) = 0;
  virtual bool launch(Slot& s, int T) = 0;

  // After open_device() and the mode's lpc_ / cpw_cap_: the chip's wave slots and the slots' events.
  bool open_sums(int N, int max_calls, size_t cells) {
    N_ = N;
    max_calls_ = std::max(1, max_calls);
    cells_ = cells;
    hipDeviceProp_t prop;
    WALKER_TRY(hipGetDeviceProperties(&prop, this->device_));
    wave_slots_ = std::max(1, prop.multiProcessorCount) * kWavesPerCu;
    for (Slot& s : slot_)
      if (!this->make_event(s.ev0) || !this->make_event(s.ev1)) return false;
    return true;
  }
  // calls per workgroup: one while every call finds a wave slot of its own on the chip, beyond that as many as fill the
  // lanes and the LDS
  Shape launch_shape(int T) const {
    const int waves_per_call = (lpc_ + 63) / 64;
    const int cpw = std::max(1, std::min(cpw_cap_, (int)(((long long)T * waves_per_call + wave_slots_ - 1) / wave_slots_)));
    return {cpw, std::max(64, cpw * lpc_), (T + cpw - 1) / cpw};
  }

  int N_ = 0, max_calls_ = 1;
  int lpc_ = 1, cpw_cap_ = 1;  // lanes per call; the calls that fit the lanes and the LDS of a workgroup
  Slot slot_[2];
  double *num_ = nullptr, *den_ = nullptr;  // [blocks][cells]

 private:
  bool wait(Slot& s) {
    if (!this->wait_event(s.ev1, s.ev0, s.ev1)) return false;
    s.busy = false;
    return true;
  }
  // the per-block sums for at least `blocks` blocks (new ones zero), in the stream's order
  bool grow(int blocks) {
    if (blocks <= cap_) {
      blocks_ = std::max(blocks_, blocks);
      return true;
    }
    const int cap = std::max(blocks, 2 * cap_);
    double *num = nullptr, *den = nullptr;
    WALKER_TRY(hipMalloc((void**)&num, sizeof(double) * cap * cells_));
    if (hipMalloc((void**)&den, sizeof(double) * cap * cells_) != hipSuccess) {
      (void)hipFree(num);
      return this->fail("hipMalloc of the per-block sums", COLATE_EHIP);
    }
    // the new pair is filled in the stream's order and takes the old one's place only once that has succeeded
    hipStream_t st = this->stream_;
    hipError_t e = hipMemsetAsync(num, 0, sizeof(double) * cap * cells_, st);
    if (e == hipSuccess) e = hipMemsetAsync(den, 0, sizeof(double) * cap * cells_, st);
    if (e == hipSuccess && blocks_) e = hipMemcpyAsync(num, num_, sizeof(double) * blocks_ * cells_, hipMemcpyDeviceToDevice, st);
    if (e == hipSuccess && blocks_) e = hipMemcpyAsync(den, den_, sizeof(double) * blocks_ * cells_, hipMemcpyDeviceToDevice, st);
    const hipError_t synced = hipStreamSynchronize(st);  // (also after a failed call: nothing may still write to the pair)
    if (e == hipSuccess) e = synced;
    if (e != hipSuccess) {
      (void)hipFree(num);
      (void)hipFree(den);
      return this->fail(std::string("growing the per-block sums: ") + hipGetErrorString(e), COLATE_EHIP);
    }
    if (num_) (void)hipFree(num_);
    if (den_) (void)hipFree(den_);
    num_ = num, den_ = den;
    cap_ = cap;
    blocks_ = blocks;
    return true;
  }

  const char* name_;  // "coalrate" / "coalrate tree": the prefix of a message
  size_t cells_ = 0;
  int wave_slots_ = 1, cur_ = 0, cap_ = 0, blocks_ = 0;
};

}  // namespace colate_cr
