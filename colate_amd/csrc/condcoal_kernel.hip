// colate_amd/csrc/condcoal_kernel.hip -- the tree walks of `Colate --mode CondCoalRates` on the GPU (condcoal.h, condcoal_walk.hpp).
//
// One workgroup per tree at a time (tree t, t + grid, ...), one lane per focal haplotype (batches of kBlock):
//   1. the per-group prefix counts over the tree's DFS leaf order (and the conditional group's, row G), a scan per row;
//   2. every lane walks its focal leaf (cc_focal_walk) and adds into its own row of the workgroup's slab in global memory
//      (no other lane writes there: plain read-modify-write, no atomics);
//   3. the workgroup sums the slab's rows in lane order into the tree's accumulators.
// The host then adds the trees' accumulators into their genome blocks in tree order: every sum has a fixed order, so two
// runs give the same bits.
#include "condcoal_device.hpp"

namespace colate_cc {
namespace {

struct KernelArgs {
  int T, N, F, S;
  const int *parent, *lo, *hi, *leaf;
  const double* bl;
  const float* factor;
  const int* focal;
  CcShared sh;
  int* pre;       // [grid][(G+1)(N+1)]
  double* slab;   // [grid][S][kBlock]
  double* out;    // [T][S]
};

__global__ __launch_bounds__(kBlock) void condcoal_kernel(KernelArgs a) {
  const int tid = threadIdx.x;
  const int N = a.N, G = a.sh.G, nn = 2 * N - 1, S = a.S;
  int* const pre = a.pre + (size_t)blockIdx.x * (G + 1) * (N + 1);
  double* const slab = a.slab + (size_t)blockIdx.x * S * kBlock;
  const int chunk = (N + kBlock - 1) / kBlock;
  const int q0 = min(N, tid * chunk), q1 = min(N, q0 + chunk);
  for (int t = blockIdx.x; t < a.T; t += gridDim.x) {
    const int* leaf = a.leaf + (size_t)t * N;
    // 1. prefix counts: a row per group, and the conditional group's
    cc_prefix_rows(N, q0, q1, G + 1, leaf, pre, [&](int row, int x) { return (row < G) ? (a.sh.group[x] == row) : (int)a.sh.is_cond[x]; });
    __threadfence_block();
    __syncthreads();
    CcTree tr;
    tr.parent = a.parent + (size_t)t * nn;
    tr.bl = a.bl + (size_t)t * nn;
    tr.lo = a.lo + (size_t)t * nn;
    tr.hi = a.hi + (size_t)t * nn;
    tr.leaf = leaf;
    tr.prefix = pre;
    tr.factor = a.factor[t];
    double* const out = a.out + (size_t)t * S;
    // 2./3. batches of kBlock focal leaves
    for (int b = 0; b < a.F; b += kBlock) {
      const int rows = min(kBlock, a.F - b);
      if (tid < rows) {
        SlabRow acc{slab + tid};
        for (int c = 0; c < S; c++) acc.p[(size_t)c * kBlock] = 0.0;
        cc_focal_walk(a.sh, tr, a.focal[b + tid], acc);
      }
      __threadfence_block();
      __syncthreads();
      for (int c = tid; c < S; c += kBlock) {
        const double* col = slab + (size_t)c * kBlock;
        double s = (b == 0) ? 0.0 : out[c];
        for (int r = 0; r < rows; r++) s += col[r];
        out[c] = s;
      }
      __threadfence_block();
      __syncthreads();
    }
  }
}

class SingleWalker final : public CcDeviceWalker {
 public:
  bool init(int device, const CcRun& run, int max_trees) {
    if (!open(device, run, max_trees, false)) return false;
    S_ = run.slots();
    F_ = (int)run.focal.size();
    grid_ = slab_grid(max_trees_, S_);
    if (!upload(d_cond_, run.is_cond) || !upload(d_focal_, run.focal)) return false;
    sh_.is_cond = d_cond_;
    sh_.cond_empty = run.cond_empty ? 1 : 0;
    WALKER_TRY(buf_.device(d_pre_, (size_t)grid_ * (run.G + 1) * (N_ + 1)));
    WALKER_TRY(buf_.device(d_slab_, (size_t)grid_ * S_ * kBlock));
    for (Result& r : res_)
      if (!make(r.out, (size_t)max_trees_ * S_)) return false;
    return true;
  }

  bool submit(const CcChunk& c) override {
    if (c.T == 0) return true;
    if (!accepts(c)) return false;
    const int k = cur_;
    cur_ ^= 1;
    if (!drain(k) || !stage(slot_[k], c, 0, c.T)) return false;
    Slot& s = slot_[k];
    Result& r = res_[k];
    r.block = c.block;
    KernelArgs a;
    a.T = c.T;
    a.N = N_;
    a.F = F_;
    a.S = S_;
    a.parent = s.parent.d;
    a.lo = s.lo.d;
    a.hi = s.hi.d;
    a.leaf = s.leaf.d;
    a.bl = s.bl.d;
    a.factor = s.factor.d;
    a.focal = d_focal_;
    a.sh = sh_;
    a.pre = d_pre_;
    a.slab = d_slab_;
    a.out = r.out.d;
    WALKER_TRY(hipEventRecord(s.ev0, stream_));
    hipLaunchKernelGGL(condcoal_kernel, dim3(std::min(grid_, c.T)), dim3(kBlock), 0, stream_, a);
    WALKER_TRY(hipGetLastError());
    WALKER_TRY(hipEventRecord(s.evk, stream_));
    WALKER_TRY(hipMemcpyAsync(r.out.h, r.out.d, sizeof(double) * c.T * S_, hipMemcpyDeviceToHost, stream_));
    WALKER_TRY(hipEventRecord(s.ev1, stream_));
    s.busy = true;
    return true;
  }

  bool finish(CcTables& acc) override {
    if (!drain(cur_) || !drain(cur_ ^ 1)) return false;
    acc.assign(1, std::move(acc_));
    acc_.clear();
    return true;
  }

 private:
  // waits for a slot's launch and adds its trees into their blocks, in tree order
  bool drain(int k) {
    Slot& s = slot_[k];
    if (!s.busy) return true;
    if (!wait(s)) return false;
    for (int t = 0; t < s.T; t++) {
      const int b = res_[k].block[t];
      if ((int)acc_.size() <= b) acc_.resize(b + 1);
      std::vector<double>& dst = acc_[b];
      if (dst.empty()) dst.assign(S_, 0.0);
      const double* src = res_[k].out.h + (size_t)t * S_;
      for (int c = 0; c < S_; c++) dst[c] += src[c];
    }
    return true;
  }

  int S_ = 0, F_ = 0, grid_ = 0;
  int* d_focal_ = nullptr;
  unsigned char* d_cond_ = nullptr;
  int* d_pre_ = nullptr;      // [grid][(G+1)(N+1)]
  double* d_slab_ = nullptr;  // [grid][S][kBlock]
  struct Result {             // of a slot's launch
    Staged<double> out;       // [T][S] per-tree accumulators
    std::vector<int> block;   // the trees' blocks
  } res_[2];
  std::vector<std::vector<double>> acc_;  // [block][S]
};

}  // namespace

std::unique_ptr<CcWalker> make_device_walker(int device, const CcRun& run, int max_trees, std::string& why) {
  auto w = std::make_unique<SingleWalker>();
  if (!w->init(device, run, max_trees)) {
    why = w->error();
    return nullptr;
  }
  return w;
}

}  // namespace colate_cc
