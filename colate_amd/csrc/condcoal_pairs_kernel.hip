// colate_amd/csrc/condcoal_pairs_kernel.hip -- the tree walks of `Colate --mode CondCoalRates --pairs` on the GPU: many
// (focal group, conditional group) pairs in one pass over the trees (condcoal.h: CcPairsDevice; the walk is
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
// Every sum is the single path's, in its order (CcDevice: lane, then focal haplotypes ascending, then trees from 0.0), so
// each pair's accumulators are bit for bit those of colate_condcoal_accumulate for that pair.  No atomics.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstring>

#include "colate_amd.h"
#include "colate_internal.h"
#include "condcoal.h"
#include "condcoal_walk.hpp"

namespace colate_cc {
namespace {

constexpr int kBlock = 256;    // lanes per workgroup = items per batch = rows of a slab
constexpr int kMaxGrid = 1024;
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

struct SlabRow {
  double* p;  // this lane's column of the slab: slot c at p[c * kBlock]
  __device__ void add(int c, double v) { p[(size_t)c * kBlock] += v; }
};

// per-group prefix counts of each tree's leaf order: per-lane chunk counts, a serial scan of the kBlock partials, per-lane
// running sums (condcoal_kernel.hip's step 1 without the conditional row)
__global__ __launch_bounds__(kBlock) void condcoal_pairs_prefix(int T, int N, int G, const int* group, const int* leaves,
                                                                int* pre_all) {
  __shared__ int s_part[kBlock];
  const int tid = threadIdx.x;
  const int chunk = (N + kBlock - 1) / kBlock;
  const int q0 = min(N, tid * chunk), q1 = min(N, q0 + chunk);
  for (int t = blockIdx.x; t < T; t += gridDim.x) {
    const int* leaf = leaves + (size_t)t * N;
    int* const pre = pre_all + (size_t)t * G * (N + 1);
    for (int row = 0; row < G; row++) {
      int cnt = 0;
      for (int q = q0; q < q1; q++) cnt += group[leaf[q]] == row;
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
        run += group[leaf[q]] == row;
      }
      __syncthreads();
    }
  }
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

#define CC_TRY(expr)                                            \
  do {                                                          \
    hipError_t e_ = (expr);                                     \
    if (e_ != hipSuccess) {                                     \
      err_ = std::string(#expr) + ": " + hipGetErrorString(e_); \
      code_ = COLATE_EHIP;                                      \
      return false;                                             \
    }                                                           \
  } while (0)

}  // namespace

struct CcPairsDevice::Impl {
  int device = 0, N = 0, G = 0, S = 0, P = 0, U = 0, W = 0, max_trees = 0, grid = 0;
  size_t PS = 0;
  CcShared sh{};
  // run constants
  int *d_group = nullptr, *d_item_hap = nullptr, *d_item_pair = nullptr, *d_pair_start = nullptr, *d_pair_cond = nullptr,
      *d_unit_start = nullptr;
  double* d_ages = nullptr;
  float *d_epochs = nullptr, *d_efocal = nullptr;
  // shared by the launches (one stream: each launch runs after the previous one)
  int* d_pre = nullptr;       // [max_trees][G][N+1]
  double* d_slab = nullptr;   // [grid][S][kBlock]
  double* d_out = nullptr;    // [max_trees][P][S]
  double* d_run = nullptr;    // [P][S] the open block's running sums
  double* d_closed = nullptr; // [kMaxCloses][P][S]
  int open_block = -1;        // the block whose sums are in d_run (-1: none yet)
  // two launch slots: pinned staging and device copies of the trees, the closed blocks coming back
  struct Slot {
    int T = 0;
    int *h_parent = nullptr, *h_lo = nullptr, *h_hi = nullptr, *h_leaf = nullptr, *h_block = nullptr;
    double* h_bl = nullptr;
    float* h_factor = nullptr;
    double* h_closed = nullptr;  // [kMaxCloses][P][S]
    std::vector<int> closed;     // the blocks of h_closed's rows
    int *d_parent = nullptr, *d_lo = nullptr, *d_hi = nullptr, *d_leaf = nullptr, *d_block = nullptr;
    double* d_bl = nullptr;
    float* d_factor = nullptr;
    hipEvent_t ev0 = nullptr, evk = nullptr, ev1 = nullptr;  // kernels start / kernels end / closed blocks copied back
    bool busy = false;
  } slot[2];
  int cur = 0;
  hipStream_t stream = nullptr;
  std::vector<std::vector<double>> acc;
};

bool CcPairsDevice::fail(const char* what, int code) {
  err_ = what;
  code_ = code;
  return false;
}

CcPairsDevice* CcPairsDevice::create(int device, const CcRun& base, const std::vector<int>& focal_group,
                                     const std::vector<int>& cond_group, int max_trees, std::string& why) {
  colate::mark_device_touched();
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) {
    why = "no HIP device";
    return nullptr;
  }
  if (device < 0 && hipGetDevice(&device) != hipSuccess) device = 0;  // -1: the calling thread's device
  if (device >= n) {
    why = "no HIP device " + std::to_string(device);
    return nullptr;
  }
  const int N = base.N, G = base.G, P = (int)focal_group.size();
  if (P < 1 || (int)cond_group.size() != P) {
    why = "no pairs";
    return nullptr;
  }
  // the items (pair after pair, each pair's focal haplotypes ascending), the pairs' conditional groups (-1 where the
  // group has no haplotype) and the work units (consecutive pairs, at most kBlock items unless one pair has more)
  std::vector<int> item_hap, item_pair, pair_start(1, 0), pair_cond(P), unit_start(1, 0);
  for (int p = 0; p < P; p++) {
    const int fg = focal_group[p], cg = cond_group[p];
    const int before = (int)item_hap.size();
    bool cond_any = false;
    for (int i = 0; i < N; i++) {
      if (base.group[i] == fg) item_hap.push_back(i), item_pair.push_back(p);
      cond_any |= base.group[i] == cg;
    }
    if ((int)item_hap.size() == before) {
      why = "pair " + std::to_string(p) + ": no focal haplotype";
      return nullptr;
    }
    pair_cond[p] = cond_any ? cg : -1;
    pair_start.push_back((int)item_hap.size());
    if (pair_start[p + 1] - unit_start.back() > kBlock && pair_start[p] > unit_start.back()) unit_start.push_back(pair_start[p]);
  }
  unit_start.push_back(pair_start[P]);
  CcPairsDevice* d = new CcPairsDevice();
  Impl* p = d->p_ = new Impl();
  p->device = device;
  p->N = N;
  p->G = G;
  p->S = base.slots();
  p->P = P;
  p->PS = (size_t)P * p->S;
  p->W = (int)item_hap.size();
  p->U = (int)unit_start.size() - 1;
  p->max_trees = std::max(1, max_trees);
  const size_t slab_bytes = (size_t)kBlock * p->S * sizeof(double);
  p->grid = (int)std::max<size_t>(1, std::min<size_t>({(size_t)kMaxGrid, (size_t)p->max_trees * p->U, ((size_t)2 << 30) / slab_bytes}));
  auto bad = [&](const std::string& w) {
    why = w;
    delete d;
    return (CcPairsDevice*)nullptr;
  };
#define CC_MK(expr)                                                                        \
  do {                                                                                     \
    hipError_t e_ = (expr);                                                                \
    if (e_ != hipSuccess) return bad(std::string(#expr) + ": " + hipGetErrorString(e_)); \
  } while (0)
#define CC_UP(dst, vec)                                                                                 \
  do {                                                                                                  \
    CC_MK(hipMalloc(&(dst), sizeof((vec)[0]) * std::max<size_t>(1, (vec).size())));                    \
    if (!(vec).empty()) CC_MK(hipMemcpy((dst), (vec).data(), sizeof((vec)[0]) * (vec).size(), hipMemcpyHostToDevice)); \
  } while (0)
  CC_MK(hipSetDevice(device));
  CC_MK(hipStreamCreateWithFlags(&p->stream, hipStreamNonBlocking));
  const int nn = 2 * N - 1;
  CC_UP(p->d_group, base.group);
  CC_UP(p->d_item_hap, item_hap);
  CC_UP(p->d_item_pair, item_pair);
  CC_UP(p->d_pair_start, pair_start);
  CC_UP(p->d_pair_cond, pair_cond);
  CC_UP(p->d_unit_start, unit_start);
  CC_UP(p->d_epochs, base.epochs);
  CC_UP(p->d_efocal, base.efocal);
  if (!base.ages.empty()) CC_UP(p->d_ages, base.ages);
#undef CC_UP
  const size_t T = p->max_trees;
  CC_MK(hipMalloc(&p->d_pre, sizeof(int) * T * G * (N + 1)));
  CC_MK(hipMalloc(&p->d_slab, slab_bytes * p->grid));
  CC_MK(hipMalloc(&p->d_out, sizeof(double) * T * p->PS));
  CC_MK(hipMalloc(&p->d_run, sizeof(double) * p->PS));
  CC_MK(hipMemset(p->d_run, 0, sizeof(double) * p->PS));
  CC_MK(hipMalloc(&p->d_closed, sizeof(double) * kMaxCloses * p->PS));
  for (auto& s : p->slot) {
    CC_MK(hipHostMalloc(&s.h_parent, sizeof(int) * T * nn, hipHostMallocDefault));
    CC_MK(hipHostMalloc(&s.h_lo, sizeof(int) * T * nn, hipHostMallocDefault));
    CC_MK(hipHostMalloc(&s.h_hi, sizeof(int) * T * nn, hipHostMallocDefault));
    CC_MK(hipHostMalloc(&s.h_leaf, sizeof(int) * T * N, hipHostMallocDefault));
    CC_MK(hipHostMalloc(&s.h_block, sizeof(int) * T, hipHostMallocDefault));
    CC_MK(hipHostMalloc(&s.h_bl, sizeof(double) * T * nn, hipHostMallocDefault));
    CC_MK(hipHostMalloc(&s.h_factor, sizeof(float) * T, hipHostMallocDefault));
    CC_MK(hipHostMalloc(&s.h_closed, sizeof(double) * kMaxCloses * p->PS, hipHostMallocDefault));
    CC_MK(hipMalloc(&s.d_parent, sizeof(int) * T * nn));
    CC_MK(hipMalloc(&s.d_lo, sizeof(int) * T * nn));
    CC_MK(hipMalloc(&s.d_hi, sizeof(int) * T * nn));
    CC_MK(hipMalloc(&s.d_leaf, sizeof(int) * T * N));
    CC_MK(hipMalloc(&s.d_block, sizeof(int) * T));
    CC_MK(hipMalloc(&s.d_bl, sizeof(double) * T * nn));
    CC_MK(hipMalloc(&s.d_factor, sizeof(float) * T));
    CC_MK(hipEventCreate(&s.ev0));
    CC_MK(hipEventCreate(&s.evk));
    CC_MK(hipEventCreate(&s.ev1));
  }
#undef CC_MK
  p->sh.N = N;
  p->sh.G = G;
  p->sh.E = base.E();
  p->sh.EF = base.EF();
  p->sh.group = p->d_group;
  p->sh.is_cond = nullptr;
  p->sh.cond_empty = 0;
  p->sh.ages = p->d_ages;
  p->sh.epochs = p->d_epochs;
  p->sh.efocal = p->d_efocal;
  return d;
}

CcPairsDevice::~CcPairsDevice() {
  if (!p_) return;
  Impl* p = p_;
  if (p->stream) (void)hipStreamSynchronize(p->stream);
  for (auto& s : p->slot) {
    for (void* h : {(void*)s.h_parent, (void*)s.h_lo, (void*)s.h_hi, (void*)s.h_leaf, (void*)s.h_block, (void*)s.h_bl,
                    (void*)s.h_factor, (void*)s.h_closed})
      if (h) (void)hipHostFree(h);
    for (void* q : {(void*)s.d_parent, (void*)s.d_lo, (void*)s.d_hi, (void*)s.d_leaf, (void*)s.d_block, (void*)s.d_bl,
                    (void*)s.d_factor})
      if (q) (void)hipFree(q);
    if (s.ev0) (void)hipEventDestroy(s.ev0);
    if (s.evk) (void)hipEventDestroy(s.evk);
    if (s.ev1) (void)hipEventDestroy(s.ev1);
  }
  for (void* q : {(void*)p->d_group, (void*)p->d_item_hap, (void*)p->d_item_pair, (void*)p->d_pair_start, (void*)p->d_pair_cond,
                  (void*)p->d_unit_start, (void*)p->d_ages, (void*)p->d_epochs, (void*)p->d_efocal, (void*)p->d_pre,
                  (void*)p->d_slab, (void*)p->d_out, (void*)p->d_run, (void*)p->d_closed})
    if (q) (void)hipFree(q);
  if (p->stream) (void)hipStreamDestroy(p->stream);
  delete p;
}

// waits for a slot's launch and keeps the blocks it closed
bool CcPairsDevice::drain(int k) {
  Impl::Slot& s = p_->slot[k];
  if (!s.busy) return true;
  CC_TRY(hipEventSynchronize(s.ev1));
  float ms = 0.f;
  if (hipEventElapsedTime(&ms, s.ev0, s.evk) == hipSuccess) gpu_s_ += ms * 1e-3;
  const size_t PS = p_->PS;
  for (size_t r = 0; r < s.closed.size(); r++) {
    const int b = s.closed[r];
    if ((int)p_->acc.size() <= b) p_->acc.resize(b + 1);
    p_->acc[b].assign(s.h_closed + r * PS, s.h_closed + (r + 1) * PS);
  }
  s.closed.clear();
  s.busy = false;
  return true;
}

// trees [t0, t1) of the chunk, which close at most kMaxCloses blocks, on the next slot
bool CcPairsDevice::launch(const CcChunk& c, int t0, int t1) {
  Impl* p = p_;
  const int k = p->cur;
  p->cur ^= 1;
  if (!drain(k)) return false;
  Impl::Slot& s = p->slot[k];
  const int N = p->N, nn = 2 * N - 1;
  const size_t T = t1 - t0;
  std::memcpy(s.h_parent, c.parent.data() + (size_t)t0 * nn, sizeof(int) * T * nn);
  std::memcpy(s.h_lo, c.lo.data() + (size_t)t0 * nn, sizeof(int) * T * nn);
  std::memcpy(s.h_hi, c.hi.data() + (size_t)t0 * nn, sizeof(int) * T * nn);
  std::memcpy(s.h_leaf, c.leaf.data() + (size_t)t0 * N, sizeof(int) * T * N);
  std::memcpy(s.h_block, c.block.data() + t0, sizeof(int) * T);
  std::memcpy(s.h_bl, c.bl.data() + (size_t)t0 * nn, sizeof(double) * T * nn);
  std::memcpy(s.h_factor, c.factor.data() + t0, sizeof(float) * T);
  s.T = (int)T;
  s.closed.clear();
  int open = p->open_block;
  for (int t = t0; t < t1; t++)
    if (c.block[t] != open) {
      if (open >= 0) s.closed.push_back(open);
      open = c.block[t];
    }
  if ((int)s.closed.size() > kMaxCloses) return fail("condcoal: a launch closes too many blocks", COLATE_EINVAL);
  CC_TRY(hipSetDevice(p->device));
  CC_TRY(hipMemcpyAsync(s.d_parent, s.h_parent, sizeof(int) * T * nn, hipMemcpyHostToDevice, p->stream));
  CC_TRY(hipMemcpyAsync(s.d_lo, s.h_lo, sizeof(int) * T * nn, hipMemcpyHostToDevice, p->stream));
  CC_TRY(hipMemcpyAsync(s.d_hi, s.h_hi, sizeof(int) * T * nn, hipMemcpyHostToDevice, p->stream));
  CC_TRY(hipMemcpyAsync(s.d_leaf, s.h_leaf, sizeof(int) * T * N, hipMemcpyHostToDevice, p->stream));
  CC_TRY(hipMemcpyAsync(s.d_block, s.h_block, sizeof(int) * T, hipMemcpyHostToDevice, p->stream));
  CC_TRY(hipMemcpyAsync(s.d_bl, s.h_bl, sizeof(double) * T * nn, hipMemcpyHostToDevice, p->stream));
  CC_TRY(hipMemcpyAsync(s.d_factor, s.h_factor, sizeof(float) * T, hipMemcpyHostToDevice, p->stream));
  PairsArgs a;
  a.T = (int)T;
  a.N = N;
  a.S = p->S;
  a.P = p->P;
  a.U = p->U;
  a.parent = s.d_parent;
  a.lo = s.d_lo;
  a.hi = s.d_hi;
  a.leaf = s.d_leaf;
  a.bl = s.d_bl;
  a.factor = s.d_factor;
  a.pre = p->d_pre;
  a.item_hap = p->d_item_hap;
  a.item_pair = p->d_item_pair;
  a.pair_start = p->d_pair_start;
  a.pair_cond = p->d_pair_cond;
  a.unit_start = p->d_unit_start;
  a.sh = p->sh;
  a.slab = p->d_slab;
  a.out = p->d_out;
  CC_TRY(hipEventRecord(s.ev0, p->stream));
  hipLaunchKernelGGL(condcoal_pairs_prefix, dim3(std::min<size_t>(T, kMaxGrid)), dim3(kBlock), 0, p->stream, (int)T, N, p->G,
                     (const int*)p->d_group, (const int*)s.d_leaf, p->d_pre);
  CC_TRY(hipGetLastError());
  const int grid = (int)std::min<size_t>(p->grid, T * p->U);
  hipLaunchKernelGGL(condcoal_pairs_kernel, dim3(grid), dim3(kBlock), 0, p->stream, a);
  CC_TRY(hipGetLastError());
  hipLaunchKernelGGL(condcoal_pairs_blocks, dim3((unsigned)((p->PS + kBlock - 1) / kBlock)), dim3(kBlock), 0, p->stream, (int)T,
                     (long)p->PS, (const int*)s.d_block, p->open_block, (const double*)p->d_out, p->d_run, p->d_closed);
  CC_TRY(hipGetLastError());
  CC_TRY(hipEventRecord(s.evk, p->stream));
  if (!s.closed.empty())
    CC_TRY(hipMemcpyAsync(s.h_closed, p->d_closed, sizeof(double) * s.closed.size() * p->PS, hipMemcpyDeviceToHost, p->stream));
  CC_TRY(hipEventRecord(s.ev1, p->stream));
  p->open_block = open;
  s.busy = true;
  return true;
}

bool CcPairsDevice::submit(const CcChunk& c) {
  Impl* p = p_;
  if (c.T == 0) return true;
  if (c.T > p->max_trees || c.N != p->N) return fail("condcoal: chunk larger than the device buffers", COLATE_EINVAL);
  // pieces that close at most kMaxCloses blocks each (blocks in non-decreasing order)
  int t0 = 0, closes = 0, open = p->open_block;
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

bool CcPairsDevice::finish(std::vector<std::vector<double>>& acc) {
  Impl* p = p_;
  if (!drain(p->cur) || !drain(p->cur ^ 1)) return false;
  if (p->open_block >= 0) {
    const int b = p->open_block;
    if ((int)p->acc.size() <= b) p->acc.resize(b + 1);
    p->acc[b].resize(p->PS);
    CC_TRY(hipSetDevice(p->device));
    CC_TRY(hipMemcpyAsync(p->acc[b].data(), p->d_run, sizeof(double) * p->PS, hipMemcpyDeviceToHost, p->stream));
    CC_TRY(hipStreamSynchronize(p->stream));
    p->open_block = -1;
  }
  acc = std::move(p->acc);
  p->acc.clear();
  return true;
}

}  // namespace colate_cc
