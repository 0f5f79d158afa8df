// colate_amd/csrc/coalrate_kernel.hip -- the pair counting of `CoalRate --mode local_ancestry` on the device (coalrate.h:
// the formulas, shared with the host twin).  Per chunk of calls, two launches on one stream:
//   * cr_count: a call's lanes stage the group label of every position of its DFS leaf order in LDS and scan it into
//     per-group prefix counts (16-bit: N <= 16384; in LDS where G * (N + 1) of them fit beside the labels in the 160 KiB a
//     workgroup may ask for, in device memory otherwise): every lane counts its stretch of positions per group, one lane
//     per group scans the stretches' counts, every lane writes its stretch of every row.  Then the lanes walk the call's
//     internal nodes, one lane per group pair, each node one 16-byte load and six prefix reads.  Calls with few group
//     pairs share a workgroup once a chunk has more calls than the chip has wave slots.  Out: cumB / R [call][E][GP].
//   * cr_fold: one lane per (epoch, group pair) cell adds the calls' addends into their blocks in call order; the
//     per-block sums stay on the device until finish().
// No atomics: every output word has one writer.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include "coalrate.h"
#include "condcoal_device.hpp"

namespace colate_cr {

namespace {

using colate_cc::CcBuffers;

constexpr int kMaxLanes = 256;            // lanes per workgroup
constexpr size_t kLdsBytes = 160 * 1024;  // the LDS of a CU, which one workgroup may have whole (the launch opts in)
constexpr int kWavesPerCu = 8;            // resident waves per CU beyond which packing calls into a workgroup pays

struct CountArgs {
  int T, N, G, E, GP;
  int cpw, lpc;  // calls per workgroup, lanes per call
  const int* leaf;       // [T][N]
  const CrNode* node;    // [T][N-1]
  const int* gv;         // [T]
  const int* groups;     // [S][N]
  unsigned short* gpre;  // [T][G][N+1] (the device-memory path)
  int* cumB;             // [T][E][GP]
  double* R;             // [T][E][GP]
};

struct LdsPre {
  const unsigned short* p;
  int n1;
  __device__ int operator()(int g, int q) const { return p[g * n1 + q]; }
};

template <bool kLds>
__global__ void __launch_bounds__(kMaxLanes) cr_count(CountArgs a) {
  extern __shared__ unsigned short s_mem[];
  const int slot = threadIdx.x / a.lpc, lane = threadIdx.x % a.lpc;
  const int k = blockIdx.x * a.cpw + slot;
  const bool active = slot < a.cpw && k < a.T;
  const int n1 = a.N + 1;
  // LDS: the labels of every slot, the per-lane group counts of every slot, then (kLds) the prefix rows of every slot
  unsigned short* lab = s_mem + (size_t)slot * a.N;
  unsigned short* cnt = s_mem + (size_t)a.cpw * a.N + (size_t)slot * a.lpc * a.G;
  unsigned short* pre = kLds ? s_mem + (size_t)a.cpw * (a.N + a.lpc * a.G) + (size_t)slot * a.G * n1
                             : a.gpre + (size_t)(active ? k : 0) * a.G * n1;
  // this lane's stretch of the leaf order
  const int len = (a.N + a.lpc - 1) / a.lpc, q0 = min(a.N, lane * len), q1 = min(a.N, q0 + len);
  if (active) {
    const int* leaf = a.leaf + (size_t)k * a.N;
    const int* grp = a.groups + (size_t)a.gv[k] * a.N;
    unsigned short* mine = cnt + (size_t)lane * a.G;
    for (int g = 0; g < a.G; g++) mine[g] = 0;
    for (int q = q0; q < q1; q++) {
      const unsigned short g = (unsigned short)grp[leaf[q]];
      lab[q] = g;
      mine[g]++;
    }
  }
  __syncthreads();
  if (active)
    for (int g = lane; g < a.G; g += a.lpc) {  // the stretches' counts of group g into their exclusive prefix
      int run = 0;
      for (int l = 0; l < a.lpc; l++) {
        const int c = cnt[l * a.G + g];
        cnt[l * a.G + g] = (unsigned short)run;
        run += c;
      }
      pre[(size_t)g * n1 + a.N] = (unsigned short)run;
    }
  __syncthreads();
  if (active)
    for (int g = 0; g < a.G; g++) {
      unsigned short* row = pre + (size_t)g * n1;
      int run = cnt[lane * a.G + g];
      for (int q = q0; q < q1; q++) {
        row[q] = (unsigned short)run;
        run += (lab[q] == g);
      }
    }
  __syncthreads();
  if (!active) return;
  const CrNode* node = a.node + (size_t)k * (a.N - 1);
  const size_t out = (size_t)k * a.E * a.GP;
  const LdsPre rd{pre, n1};
  for (int gp = lane; gp < a.GP; gp += a.lpc) {
    int g1 = 0;
    while (cr_pair(g1 + 1, 0) <= gp) g1++;
    const int g2 = gp - cr_pair(g1, 0);
    cr_count_pair(a.N - 1, a.E, node, g1, g2, rd, a.cumB + out + gp, a.R + out + gp, (size_t)a.GP);
  }
}

struct FoldArgs {
  int T, E, GP, OA;
  const int* cumB;
  const double* R;
  const double* w;
  const int* gv;
  const int* block;
  const int* oa_epoch;       // [OA]
  const long long* pairs;    // [S][OA][GP]
  const double* sub;         // [S][OA][GP]
  const double* width;       // [E]
  double* num;               // [blocks][E][GP]
  double* den;
};

__global__ void __launch_bounds__(kMaxLanes) cr_fold(FoldArgs a) {
  const int cell = blockIdx.x * blockDim.x + threadIdx.x;
  const int cells = a.E * a.GP;
  if (cell >= cells) return;
  const int e = cell / a.GP, gp = cell % a.GP;
  const double width = a.width[e];
  int cur = -1;
  double num = 0.0, den = 0.0;
  for (int k = 0; k < a.T; k++) {
    const int b = a.block[k];
    if (b != cur) {
      if (cur >= 0) {
        a.num[(size_t)cur * cells + cell] = num;
        a.den[(size_t)cur * cells + cell] = den;
      }
      cur = b;
      num = a.num[(size_t)cur * cells + cell];
      den = a.den[(size_t)cur * cells + cell];
    }
    const size_t at = (size_t)k * cells + cell;
    const int cb = a.cumB[at], cb_prev = e ? a.cumB[at - a.GP] : 0;
    const size_t tab = (size_t)a.gv[k] * a.OA * a.GP + gp;
    long long ca = 0;
    double sub = 0.0;
    for (int o = 0; o < a.OA; o++) {
      const int oe = a.oa_epoch[o];
      if (oe <= e) ca += a.pairs[tab + (size_t)o * a.GP];
      if (oe == e) sub = a.sub[tab + (size_t)o * a.GP];
    }
    cr_fold_cell(cb, cb_prev, ca, a.R[at], sub, width, a.w[k], num, den);
  }
  if (cur >= 0) {
    a.num[(size_t)cur * cells + cell] = num;
    a.den[(size_t)cur * cells + cell] = den;
  }
}

#define CR_TRY(expr)                                                                                   \
  do {                                                                                                 \
    hipError_t e_ = (expr);                                                                            \
    if (e_ != hipSuccess) return fail(std::string(#expr) + ": " + hipGetErrorString(e_), COLATE_EHIP); \
  } while (0)

class DeviceWalker final : public CoalRateWalker {
 public:
  ~DeviceWalker() override {
    if (stream_) (void)hipStreamSynchronize(stream_);  // (before the buffers go)
    for (Slot& s : slot_)
      for (hipEvent_t e : {s.ev0, s.ev1})
        if (e) (void)hipEventDestroy(e);
    if (stream_) (void)hipStreamDestroy(stream_);
    if (num_) (void)hipFree(num_);
    if (den_) (void)hipFree(den_);
  }

  bool open(int device, const CrRun& run, const CrTables& tab, int max_calls) {
    colate::mark_device_touched();
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return fail("no HIP device", COLATE_EHIP);
    if (device < 0 && hipGetDevice(&device) != hipSuccess) device = 0;
    if (device >= n) return fail("no HIP device " + std::to_string(device), COLATE_EHIP);
    device_ = device;
    N_ = run.N, G_ = run.G, E_ = run.E(), GP_ = run.GP(), OA_ = tab.OA;
    max_calls_ = std::max(1, max_calls);
    lpc_ = 1;
    while (lpc_ < GP_ && lpc_ < kMaxLanes) lpc_ *= 2;
    // LDS per call: labels, per-lane group counts, and the prefix rows where all of it fits
    const size_t lab_bytes = sizeof(unsigned short) * ((size_t)N_ + (size_t)lpc_ * G_);
    const size_t pre_bytes = sizeof(unsigned short) * G_ * ((size_t)N_ + 1);
    if (lab_bytes > kLdsBytes) return fail("the labels and group counts of one tree do not fit the LDS", COLATE_ELIMIT);
    lds_pre_ = lab_bytes + pre_bytes <= kLdsBytes;
    call_lds_ = lab_bytes + (lds_pre_ ? pre_bytes : 0);
    cpw_cap_ = (int)std::max<size_t>(1, std::min<size_t>(kMaxLanes / lpc_, kLdsBytes / call_lds_));
    CR_TRY(hipSetDevice(device));
    CR_TRY(hipStreamCreateWithFlags(&stream_, hipStreamNonBlocking));
    hipDeviceProp_t prop;
    CR_TRY(hipGetDeviceProperties(&prop, device));
    wave_slots_ = std::max(1, prop.multiProcessorCount) * kWavesPerCu;
    CR_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&cr_count<true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsBytes));
    CR_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&cr_count<false>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsBytes));
    if (!upload(groups_, run.groups) || !upload(oa_epoch_, tab.oa_epoch) || !upload(pairs_, tab.pairs) || !upload(sub_, tab.sub) ||
        !upload(width_, tab.width))
      return false;
    const size_t T = max_calls_, cells = (size_t)E_ * GP_;
    for (Slot& s : slot_) {
      CR_TRY(buf_.pinned(s.h_leaf, T * N_));
      CR_TRY(buf_.pinned(s.h_node, T * (N_ - 1)));
      CR_TRY(buf_.pinned(s.h_w, T));
      CR_TRY(buf_.pinned(s.h_gv, T));
      CR_TRY(buf_.pinned(s.h_block, T));
      CR_TRY(buf_.device(s.leaf, T * N_));
      CR_TRY(buf_.device(s.node, T * (N_ - 1)));
      CR_TRY(buf_.device(s.w, T));
      CR_TRY(buf_.device(s.gv, T));
      CR_TRY(buf_.device(s.block, T));
      CR_TRY(hipEventCreate(&s.ev0));
      CR_TRY(hipEventCreate(&s.ev1));
    }
    // the kernels' intermediate results are used within the stream's order: one copy serves both slots
    CR_TRY(buf_.device(cumB_, T * cells));
    CR_TRY(buf_.device(R_, T * cells));
    if (!lds_pre_) CR_TRY(buf_.device(gpre_, T * G_ * (N_ + 1)));
    return true;
  }

  bool submit(const CrChunk& c) override {
    if (c.T == 0) return true;
    if (c.N != N_) return fail("coalrate: chunk of another N", COLATE_EINVAL);
    CR_TRY(hipSetDevice(device_));
    int max_block = 0;
    for (int k = 0; k < c.T; k++) max_block = std::max(max_block, c.block[k]);
    if (!grow(max_block + 1)) return false;
    for (int t0 = 0; t0 < c.T; t0 += max_calls_) {
      const int T = std::min(c.T - t0, max_calls_);
      Slot& s = slot_[cur_];
      cur_ ^= 1;
      if (s.busy && !wait(s)) return false;
      const size_t N = N_;
      std::memcpy(s.h_leaf, c.leaf.data() + t0 * N, sizeof(int) * T * N);
      std::memcpy(s.h_node, c.node.data() + t0 * (N - 1), sizeof(CrNode) * T * (N - 1));
      std::memcpy(s.h_w, c.w.data() + t0, sizeof(double) * T);
      std::memcpy(s.h_gv, c.gv.data() + t0, sizeof(int) * T);
      std::memcpy(s.h_block, c.block.data() + t0, sizeof(int) * T);
      CR_TRY(hipMemcpyAsync(s.leaf, s.h_leaf, sizeof(int) * T * N, hipMemcpyHostToDevice, stream_));
      CR_TRY(hipMemcpyAsync(s.node, s.h_node, sizeof(CrNode) * T * (N - 1), hipMemcpyHostToDevice, stream_));
      CR_TRY(hipMemcpyAsync(s.w, s.h_w, sizeof(double) * T, hipMemcpyHostToDevice, stream_));
      CR_TRY(hipMemcpyAsync(s.gv, s.h_gv, sizeof(int) * T, hipMemcpyHostToDevice, stream_));
      CR_TRY(hipMemcpyAsync(s.block, s.h_block, sizeof(int) * T, hipMemcpyHostToDevice, stream_));
      CR_TRY(hipEventRecord(s.ev0, stream_));
      // calls per workgroup: one while every call finds a wave slot of its own on the chip, beyond that as many as fill
      // the lanes and the LDS
      const int waves_per_call = (lpc_ + 63) / 64;
      const int cpw = std::max(1, std::min(cpw_cap_, (int)(((long long)T * waves_per_call + wave_slots_ - 1) / wave_slots_)));
      CountArgs ca{T, N_, G_, E_, GP_, cpw, lpc_, s.leaf, s.node, s.gv, groups_, gpre_, cumB_, R_};
      const int lanes = std::max(64, cpw * lpc_);
      const int grid = (T + cpw - 1) / cpw;
      const size_t lds = call_lds_ * cpw;
      if (lds_pre_) hipLaunchKernelGGL(cr_count<true>, dim3(grid), dim3(lanes), lds, stream_, ca);
      else hipLaunchKernelGGL(cr_count<false>, dim3(grid), dim3(lanes), lds, stream_, ca);
      CR_TRY(hipGetLastError());
      FoldArgs fa{T, E_, GP_, OA_, cumB_, R_, s.w, s.gv, s.block, oa_epoch_, pairs_, sub_, width_, num_, den_};
      const int cells = E_ * GP_;
      hipLaunchKernelGGL(cr_fold, dim3((cells + 63) / 64), dim3(64), 0, stream_, fa);
      CR_TRY(hipGetLastError());
      CR_TRY(hipEventRecord(s.ev1, stream_));
      s.busy = true;
    }
    return true;
  }

  bool finish(CrSums& out) override {
    CR_TRY(hipSetDevice(device_));
    for (Slot& s : slot_)
      if (s.busy && !wait(s)) return false;
    CR_TRY(hipStreamSynchronize(stream_));
    const size_t n = (size_t)blocks_ * E_ * GP_;
    out.blocks = blocks_;
    out.num.assign(n, 0.0);
    out.den.assign(n, 0.0);
    if (n) {
      CR_TRY(hipMemcpy(out.num.data(), num_, sizeof(double) * n, hipMemcpyDeviceToHost));
      CR_TRY(hipMemcpy(out.den.data(), den_, sizeof(double) * n, hipMemcpyDeviceToHost));
    }
    return true;
  }

 private:
  struct Slot {
    int *h_leaf = nullptr, *h_gv = nullptr, *h_block = nullptr, *leaf = nullptr, *gv = nullptr, *block = nullptr;
    CrNode *h_node = nullptr, *node = nullptr;
    double *h_w = nullptr, *w = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;  // kernels start / kernels end
    bool busy = false;
  };
  template <class T>
  bool upload(T*& dst, const std::vector<T>& v) {
    CR_TRY(buf_.device(dst, v.size()));
    if (!v.empty()) CR_TRY(hipMemcpy(dst, v.data(), sizeof(T) * v.size(), hipMemcpyHostToDevice));
    return true;
  }
  bool wait(Slot& s) {
    CR_TRY(hipEventSynchronize(s.ev1));
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, s.ev0, s.ev1) == hipSuccess) gpu_s_ += ms * 1e-3;
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
    const size_t cells = (size_t)E_ * GP_;
    double *num = nullptr, *den = nullptr;
    CR_TRY(hipMalloc((void**)&num, sizeof(double) * cap * cells));
    if (hipMalloc((void**)&den, sizeof(double) * cap * cells) != hipSuccess) {
      (void)hipFree(num);
      return fail("hipMalloc of the per-block sums", COLATE_EHIP);
    }
    double* old_num = num_;
    double* old_den = den_;
    num_ = num, den_ = den;
    CR_TRY(hipMemsetAsync(num_, 0, sizeof(double) * cap * cells, stream_));
    CR_TRY(hipMemsetAsync(den_, 0, sizeof(double) * cap * cells, stream_));
    if (blocks_) {
      CR_TRY(hipMemcpyAsync(num_, old_num, sizeof(double) * blocks_ * cells, hipMemcpyDeviceToDevice, stream_));
      CR_TRY(hipMemcpyAsync(den_, old_den, sizeof(double) * blocks_ * cells, hipMemcpyDeviceToDevice, stream_));
    }
    CR_TRY(hipStreamSynchronize(stream_));
    if (old_num) (void)hipFree(old_num);
    if (old_den) (void)hipFree(old_den);
    cap_ = cap;
    blocks_ = blocks;
    return true;
  }

  int device_ = 0, N_ = 0, G_ = 0, E_ = 0, GP_ = 0, OA_ = 0, max_calls_ = 1, lpc_ = 1, cpw_cap_ = 1;
  bool lds_pre_ = true;
  size_t call_lds_ = 0;
  int wave_slots_ = 1;
  CcBuffers buf_;
  hipStream_t stream_ = nullptr;
  Slot slot_[2];
  int cur_ = 0;
  int* groups_ = nullptr;
  int* oa_epoch_ = nullptr;
  long long* pairs_ = nullptr;
  double *sub_ = nullptr, *width_ = nullptr;
  int* cumB_ = nullptr;
  double* R_ = nullptr;
  unsigned short* gpre_ = nullptr;
  double *num_ = nullptr, *den_ = nullptr;
  int cap_ = 0, blocks_ = 0;
};

}  // namespace

std::unique_ptr<CoalRateWalker> make_device_walker(int device, const CrRun& run, const CrTables& tab, int max_calls, std::string& why,
                                                   int* code) {
  auto w = std::make_unique<DeviceWalker>();
  if (!w->open(device, run, tab, max_calls)) {
    why = w->error();
    if (code) *code = w->error_code();
    return nullptr;
  }
  return w;
}

}  // namespace colate_cr
