// colate_amd/csrc/condcoal_pairs_kernel.hip -- the tree walks of `Colate --mode CondCoalRates --pairs` on the GPU: many
// (focal group, conditional group) pairs in one pass over the trees (condcoal.h: make_pairs_device_walker; the walk is
// condcoal_walk.hpp's, as in condcoal_kernel.hip).
//
// A lane walks one (pair, focal haplotype) item.  The items are the pairs' focal haplotypes, pair after pair, each pair's
// ascending; consecutive pairs are packed into work units of at most kBlock items (a larger pair is a unit of its own),
// so one workgroup holds the lanes of several pairs and no pair is split over workgroups.  Per chunk of trees:
//   1. condcoal_pairs_prefix: the per-group prefix counts of every tree's DFS leaf order, G rows, once for all pairs (a
//      pair's conditional row is its conditional group's);
//   2. condcoal_pairs_kernel: one workgroup per (tree, unit) at a time; every lane adds into its own row of the
//      workgroup's slab (global memory, plain read-modify-write), then the workgroup sums each pair's rows in item order
//      into the tree's accumulators [T][P][S] (a pair that spans batches continues where the last batch left it);
//   3. condcoal_pairs_blocks: a thread per (pair, slot) adds the trees into the running sum of their genome block in
//      tree order; a block that closes goes to the `closed` rows, the open one stays in `run` for the next chunk.
// Every sum is the single path's, in its order (condcoal_kernel.hip: lane, then focal haplotypes ascending, then trees from 0.0), so
// each pair's accumulators are bit for bit those of colate_condcoal_accumulate for that pair.  No atomics.
#include "condcoal_device.hpp"

namespace colate_cc {
namespace {

constexpr int kMaxCloses = 4;  // blocks that one launch may close (a chunk with more is launched in pieces)

struct PairsArgs {
  int T, N, S, P, U;
  const int *parent, *lo, *hi, *leaf;
  const double* bl;
  const float* factor;
  const int* pre;         // [T][G][N+1]
  const int* item_hap;    // [W] focal haplotype of each item
  const int* item_pair;   // [W]
  const int* pair_start;  // [P+1] first item of each pair
  const int* pair_cond;   // [P] conditional group, -1: the empty group
  const int* unit_start;  // [U+1] first item of each unit (at a pair's start)
  CcShared sh;            // (is_cond and cond_empty: per pair)
  double* slab;           // [grid][S][kBlock]
  double* out;            // [T][P][S]
};

// per-group prefix counts of each tree's leaf order (condcoal_kernel.hip's step 1 without the conditional row)
__global__ __launch_bounds__(kBlock) void condcoal_pairs_prefix(int T, int N, int G, const int* group, const int* leaves,
                                                                int* pre_all) {
  const int tid = threadIdx.x;
  const int chunk = (N + kBlock - 1) / kBlock;
  const int q0 = min(N, tid * chunk), q1 = min(N, q0 + chunk);
  for (int t = blockIdx.x; t < T; t += gridDim.x)
    cc_prefix_rows(N, q0, q1, G, leaves + (size_t)t * N, pre_all + (size_t)t * G * (N + 1), [&](int row, int x) { return group[x] == row; });
}

__global__ __launch_bounds__(kBlock) void condcoal_pairs_kernel(PairsArgs a) {
  const int tid = threadIdx.x;
  const int N = a.N, G = a.sh.G, nn = 2 * N - 1, S = a.S;
  double* const slab = a.slab + (size_t)blockIdx.x * S * kBlock;
  const long work = (long)a.T * a.U;
  for (long u = blockIdx.x; u < work; u += gridDim.x) {
    const int t = (int)(u / a.U), j = (int)(u % a.U);
    CcTree tr;
    tr.parent = a.parent + (size_t)t * nn;
    tr.bl = a.bl + (size_t)t * nn;
    tr.lo = a.lo + (size_t)t * nn;
    tr.hi = a.hi + (size_t)t * nn;
    tr.leaf = a.leaf + (size_t)t * N;
    tr.prefix = a.pre + (size_t)t * G * (N + 1);
    tr.factor = a.factor[t];
    double* const out = a.out + (size_t)t * a.P * S;
    const int i0 = a.unit_start[j], i1 = a.unit_start[j + 1];
    for (int b = i0; b < i1; b += kBlock) {
      const int rows = min(kBlock, i1 - b);
      if (tid < rows) {
        const int it = b + tid, f = a.item_hap[it], cg = a.pair_cond[a.item_pair[it]];
        SlabRow acc{slab + tid};
        for (int c = 0; c < S; c++) acc.p[(size_t)c * kBlock] = 0.0;
        CcShared sh = a.sh;
        sh.cond_empty = cg < 0 ? 1 : 0;
        cc_focal_walk_cond(sh, tr, f, tr.prefix + (size_t)max(cg, 0) * (N + 1), (cg >= 0 && sh.group[f] == cg) ? 1 : 0, acc);
      }
      __threadfence_block();
      __syncthreads();
      const int p0 = a.item_pair[b], p1 = a.item_pair[b + rows - 1];
      for (int c = tid; c < S; c += kBlock) {
        const double* col = slab + (size_t)c * kBlock;
        for (int p = p0; p <= p1; p++) {
          const int ps = a.pair_start[p];
          const int r0 = max(b, ps) - b, r1 = min(b + rows, a.pair_start[p + 1]) - b;
          double* o = out + (size_t)p * S + c;
          double s = (ps >= b) ? 0.0 : *o;
          for (int r = r0; r < r1; r++) s += col[r];
          *o = s;
        }
      }
      __threadfence_block();
      __syncthreads();
    }
  }
}

// a thread per (pair, slot): the trees' sums into their blocks, in tree order
__global__ __launch_bounds__(kBlock) void condcoal_pairs_blocks(int T, long PS, const int* block, int open_block,
                                                                const double* out, double* run, double* closed) {
  const long i = (long)blockIdx.x * kBlock + threadIdx.x;
  if (i >= PS) return;
  double s = run[i];
  int cur = open_block, k = 0;
  for (int t = 0; t < T; t++) {
    const int b = block[t];
    if (b != cur) {
      if (cur >= 0 && k < kMaxCloses) closed[(size_t)k * PS + i] = s;
      k += cur >= 0;
      s = 0.0;
      cur = b;
    }
    s += out[(size_t)t * PS + i];
  }
  run[i] = s;
}


class PairsWalker final : public CcDeviceWalker {
 public:
  bool init(int device, const CcRun& base, const std::vector<int>& focal_group, const std::vector<int>& cond_group,
            int max_trees) {
    const int N = base.N;
    P_ = (int)focal_group.size();
    if (P_ < 1 || (int)cond_group.size() != P_) return fail("no pairs", COLATE_EINVAL);
    // the items (pair after pair, each pair's focal haplotypes ascending), the pairs' conditional groups (-1 where the
    // group has no haplotype) and the work units (consecutive pairs, at most kBlock items unless one pair has more)
    std::vector<int> item_hap, item_pair, pair_start(1, 0), pair_cond(P_), unit_start(1, 0);
    for (int p = 0; p < P_; p++) {
      const int fg = focal_group[p], cg = cond_group[p];
      const int before = (int)item_hap.size();
      bool cond_any = false;
      for (int i = 0; i < N; i++) {
        if (base.group[i] == fg) item_hap.push_back(i), item_pair.push_back(p);
        cond_any |= base.group[i] == cg;
      }
      if ((int)item_hap.size() == before) return fail("pair " + std::to_string(p) + ": no focal haplotype", COLATE_EINVAL);
      pair_cond[p] = cond_any ? cg : -1;
      pair_start.push_back((int)item_hap.size());
      if (pair_start[p + 1] - unit_start.back() > kBlock && pair_start[p] > unit_start.back()) unit_start.push_back(pair_start[p]);
    }
    unit_start.push_back(pair_start[P_]);
    if (!open(device, base, max_trees, true)) return false;
    G_ = base.G;
    S_ = base.slots();
    PS_ = (size_t)P_ * S_;
    U_ = (int)unit_start.size() - 1;
    grid_ = slab_grid((size_t)max_trees_ * U_, S_);
    if (!upload(d_item_hap_, item_hap) || !upload(d_item_pair_, item_pair) || !upload(d_pair_start_, pair_start) ||
        !upload(d_pair_cond_, pair_cond) || !upload(d_unit_start_, unit_start))
      return false;
    const size_t T = max_trees_;
    WALKER_TRY(buf_.device(d_pre_, T * G_ * (N + 1)));
    WALKER_TRY(buf_.device(d_slab_, (size_t)grid_ * S_ * kBlock));
    WALKER_TRY(buf_.device(d_out_, T * PS_));
    WALKER_TRY(buf_.device(d_run_, PS_));
    WALKER_TRY(hipMemset(d_run_, 0, sizeof(double) * PS_));
    WALKER_TRY(buf_.device(d_closed_, kMaxCloses * PS_));
    for (Result& r : res_) WALKER_TRY(buf_.pinned(r.h_closed, kMaxCloses * PS_));
    return true;
  }

  bool submit(const CcChunk& c) override {
    if (c.T == 0) return true;
    if (!accepts(c)) return false;
    // pieces that close at most kMaxCloses blocks each (blocks in non-decreasing order)
    int t0 = 0, closes = 0, open = open_block_;
    for (int t = 0; t < c.T; t++) {
      const int b = c.block[t];
      if (b < 0 || b < open) return fail("condcoal: the trees' blocks decrease", COLATE_EINVAL);
      if (b != open) {
        if (open >= 0 && closes == kMaxCloses) {
          if (!launch(c, t0, t)) return false;
          t0 = t;
          closes = 0;
        }
        closes += open >= 0;
        open = b;
      }
    }
    return launch(c, t0, c.T);
  }

  bool finish(CcTables& acc) override {
    if (!drain(cur_) || !drain(cur_ ^ 1)) return false;
    if (open_block_ >= 0) {
      const int b = open_block_;
      if ((int)acc_.size() <= b) acc_.resize(b + 1);
      acc_[b].resize(PS_);
      WALKER_TRY(hipSetDevice(device_));
      WALKER_TRY(hipMemcpyAsync(acc_[b].data(), d_run_, sizeof(double) * PS_, hipMemcpyDeviceToHost, stream_));
      WALKER_TRY(hipStreamSynchronize(stream_));
      open_block_ = -1;
    }
    acc.assign(P_, std::vector<std::vector<double>>(acc_.size()));
    for (int p = 0; p < P_; p++)
      for (size_t b = 0; b < acc_.size(); b++)
        if (!acc_[b].empty()) acc[p][b].assign(acc_[b].begin() + (size_t)p * S_, acc_[b].begin() + (size_t)(p + 1) * S_);
    acc_.clear();
    return true;
  }

 private:
  // waits for a slot's launch and keeps the blocks it closed
  bool drain(int k) {
    Slot& s = slot_[k];
    if (!s.busy) return true;
    if (!wait(s)) return false;
    Result& r = res_[k];
    for (size_t i = 0; i < r.closed.size(); i++) {
      const int b = r.closed[i];
      if ((int)acc_.size() <= b) acc_.resize(b + 1);
      acc_[b].assign(r.h_closed + i * PS_, r.h_closed + (i + 1) * PS_);
    }
    r.closed.clear();
    return true;
  }

  // trees [t0, t1) of the chunk, which close at most kMaxCloses blocks, on the next slot
  bool launch(const CcChunk& c, int t0, int t1) {
    const int k = cur_;
    cur_ ^= 1;
    if (!drain(k)) return false;
    Slot& s = slot_[k];
    Result& r = res_[k];
    r.closed.clear();
    int open = open_block_;
    for (int t = t0; t < t1; t++)
      if (c.block[t] != open) {
        if (open >= 0) r.closed.push_back(open);
        open = c.block[t];
      }
    if ((int)r.closed.size() > kMaxCloses) return fail("condcoal: a launch closes too many blocks", COLATE_EINVAL);
    if (!stage(s, c, t0, t1)) return false;
    const size_t T = t1 - t0;
    PairsArgs a;
    a.T = (int)T;
    a.N = N_;
    a.S = S_;
    a.P = P_;
    a.U = U_;
    a.parent = s.parent.d;
    a.lo = s.lo.d;
    a.hi = s.hi.d;
    a.leaf = s.leaf.d;
    a.bl = s.bl.d;
    a.factor = s.factor.d;
    a.pre = d_pre_;
    a.item_hap = d_item_hap_;
    a.item_pair = d_item_pair_;
    a.pair_start = d_pair_start_;
    a.pair_cond = d_pair_cond_;
    a.unit_start = d_unit_start_;
    a.sh = sh_;
    a.slab = d_slab_;
    a.out = d_out_;
    WALKER_TRY(hipEventRecord(s.ev0, stream_));
    hipLaunchKernelGGL(condcoal_pairs_prefix, dim3(std::min<size_t>(T, kMaxGrid)), dim3(kBlock), 0, stream_, (int)T, N_, G_,
                       sh_.group, (const int*)s.leaf.d, d_pre_);
    WALKER_TRY(hipGetLastError());
    const int grid = (int)std::min<size_t>(grid_, T * U_);
    hipLaunchKernelGGL(condcoal_pairs_kernel, dim3(grid), dim3(kBlock), 0, stream_, a);
    WALKER_TRY(hipGetLastError());
    hipLaunchKernelGGL(condcoal_pairs_blocks, dim3((unsigned)((PS_ + kBlock - 1) / kBlock)), dim3(kBlock), 0, stream_, (int)T,
                       (long)PS_, (const int*)s.block.d, open_block_, (const double*)d_out_, d_run_, d_closed_);
    WALKER_TRY(hipGetLastError());
    WALKER_TRY(hipEventRecord(s.evk, stream_));
    if (!r.closed.empty())
      WALKER_TRY(hipMemcpyAsync(r.h_closed, d_closed_, sizeof(double) * r.closed.size() * PS_, hipMemcpyDeviceToHost, stream_));
    WALKER_TRY(hipEventRecord(s.ev1, stream_));
    open_block_ = open;
    s.busy = true;
    return true;
  }

  int G_ = 0, S_ = 0, P_ = 0, U_ = 0, grid_ = 0;
  size_t PS_ = 0;
  int *d_item_hap_ = nullptr, *d_item_pair_ = nullptr, *d_pair_start_ = nullptr, *d_pair_cond_ = nullptr, *d_unit_start_ = nullptr;
  // shared by the launches (one stream: each launch runs after the previous one)
  int* d_pre_ = nullptr;        // [max_trees][G][N+1]
  double* d_slab_ = nullptr;    // [grid][S][kBlock]
  double* d_out_ = nullptr;     // [max_trees][P][S]
  double* d_run_ = nullptr;     // [P][S] the open block's running sums
  double* d_closed_ = nullptr;  // [kMaxCloses][P][S]
  int open_block_ = -1;         // the block whose sums are in d_run (-1: none yet)
  struct Result {               // of a slot's launch: the blocks it closed, coming back
    double* h_closed = nullptr;  // [kMaxCloses][P][S]
    std::vector<int> closed;     // the blocks of h_closed's rows
  } res_[2];
  std::vector<std::vector<double>> acc_;  // [block][P][S]
};

}  // namespace

std::unique_ptr<CcWalker> make_pairs_device_walker(int device, const CcRun& base, const std::vector<int>& focal_group,
                                                   const std::vector<int>& cond_group, int max_trees, std::string& why) {
  auto w = std::make_unique<PairsWalker>();
  if (!w->init(device, base, focal_group, cond_group, max_trees)) {
    why = w->error();
    return nullptr;
  }
  return w;
}

}  // namespace colate_cc
