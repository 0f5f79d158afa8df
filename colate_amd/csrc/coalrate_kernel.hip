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
// No atomics: every output word has one writer.  The walker around the two launches is coalrate_device.hpp's.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include "coalrate_device.hpp"

namespace colate_cr {

namespace {

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

struct CrArrays {  // the calls of one launch
  Staged<int> leaf, gv, block;
  Staged<CrNode> node;
  Staged<double> w;
};

class DeviceWalker final : public BlockSumDeviceWalker<CrChunk, CrArrays> {
 public:
  DeviceWalker() : BlockSumDeviceWalker("coalrate") {}

  bool open(int device, const CrRun& run, const CrTables& tab, int max_calls) {
    if (!open_device(device)) return false;
    G_ = run.G, E_ = run.E(), GP_ = run.GP(), OA_ = tab.OA;
    const size_t N = run.N;
    lpc_ = 1;
    while (lpc_ < GP_ && lpc_ < kMaxLanes) lpc_ *= 2;
    // LDS per call: labels, per-lane group counts, and the prefix rows where all of it fits
    const size_t lab_bytes = sizeof(unsigned short) * (N + (size_t)lpc_ * G_);
    const size_t pre_bytes = sizeof(unsigned short) * G_ * (N + 1);
    if (lab_bytes > kLdsBytes) return fail("the labels and group counts of one tree do not fit the LDS", COLATE_ELIMIT);
    lds_pre_ = lab_bytes + pre_bytes <= kLdsBytes;
    call_lds_ = lab_bytes + (lds_pre_ ? pre_bytes : 0);
    cpw_cap_ = (int)std::max<size_t>(1, std::min<size_t>(kMaxLanes / lpc_, kLdsBytes / call_lds_));
    const size_t cells = (size_t)E_ * GP_;
    if (!open_sums(run.N, max_calls, cells)) return false;
    WALKER_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&cr_count<true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsBytes));
    WALKER_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&cr_count<false>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsBytes));
    if (!upload(groups_, run.groups) || !upload(oa_epoch_, tab.oa_epoch) || !upload(pairs_, tab.pairs) || !upload(sub_, tab.sub) ||
        !upload(width_, tab.width))
      return false;
    const size_t T = max_calls_;
    for (Slot& s : slot_)
      if (!make(s.leaf, T * N) || !make(s.node, T * (N - 1)) || !make(s.w, T) || !make(s.gv, T) || !make(s.block, T)) return false;
    // the kernels' intermediate results are used within the stream's order: one copy serves both slots
    WALKER_TRY(buf_.device(cumB_, T * cells));
    WALKER_TRY(buf_.device(R_, T * cells));
    if (!lds_pre_) WALKER_TRY(buf_.device(gpre_, T * G_ * (N + 1)));
    return true;
  }

 private:
  bool stage(Slot& s, const CrChunk& c, int t0, int T) override {
    const size_t N = N_;
    return send(s.leaf, c.leaf.data() + t0 * N, T * N) && send(s.node, c.node.data() + t0 * (N - 1), T * (N - 1)) &&
           send(s.w, c.w.data() + t0, T) && send(s.gv, c.gv.data() + t0, T) && send(s.block, c.block.data() + t0, T);
  }
  bool launch(Slot& s, int T) override {
    const Shape sh = launch_shape(T);
    CountArgs ca{T, N_, G_, E_, GP_, sh.cpw, lpc_, s.leaf.d, s.node.d, s.gv.d, groups_, gpre_, cumB_, R_};
    const size_t lds = call_lds_ * sh.cpw;
    if (lds_pre_) hipLaunchKernelGGL(cr_count<true>, dim3(sh.grid), dim3(sh.lanes), lds, stream_, ca);
    else hipLaunchKernelGGL(cr_count<false>, dim3(sh.grid), dim3(sh.lanes), lds, stream_, ca);
    WALKER_TRY(hipGetLastError());
    launch_stats(kLaunchLocalAncestry).note(sh.cpw, lpc_, lds_pre_);
    FoldArgs fa{T, E_, GP_, OA_, cumB_, R_, s.w.d, s.gv.d, s.block.d, oa_epoch_, pairs_, sub_, width_, num_, den_};
    const int cells = E_ * GP_;
    hipLaunchKernelGGL(cr_fold, dim3((cells + 63) / 64), dim3(64), 0, stream_, fa);
    WALKER_TRY(hipGetLastError());
    return true;
  }

  int G_ = 0, E_ = 0, GP_ = 0, OA_ = 0;
  bool lds_pre_ = true;
  size_t call_lds_ = 0;
  int* groups_ = nullptr;
  int* oa_epoch_ = nullptr;
  long long* pairs_ = nullptr;
  double *sub_ = nullptr, *width_ = nullptr;
  int* cumB_ = nullptr;
  double* R_ = nullptr;
  unsigned short* gpre_ = nullptr;
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
