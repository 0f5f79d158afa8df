// colate_amd/csrc/condcoal_kernel.hip -- the tree walks of `Colate --mode CondCoalRates` on the GPU (condcoal.h, condcoal_walk.hpp).
//
// One workgroup per tree at a time (tree t, t + grid, ...), one lane per focal haplotype (batches of kBlock):
//   1. the per-group prefix counts over the tree's DFS leaf order (and the conditional group's, row G), a scan per row;
//   2. every lane walks its focal leaf (cc_focal_walk) and adds into its own row of the workgroup's slab in global memory
//      (no other lane writes there: plain read-modify-write, no atomics);
//   3. the workgroup sums the slab's rows in lane order into the tree's accumulators.
// The host then adds the trees' accumulators into their genome blocks in tree order: every sum has a fixed order, so two
// runs give the same bits.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstring>

#include "colate_amd.h"
#include "colate_internal.h"
#include "condcoal.h"
#include "condcoal_walk.hpp"

namespace colate_cc {
namespace {

constexpr int kBlock = 256;  // lanes per workgroup = focal leaves per batch = rows of a slab
constexpr int kMaxGrid = 1024;

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

struct SlabRow {
  double* p;  // this lane's column of the slab: slot c at p[c * kBlock]
  __device__ void add(int c, double v) { p[(size_t)c * kBlock] += v; }
};

__global__ __launch_bounds__(kBlock) void condcoal_kernel(KernelArgs a) {
  __shared__ int s_part[kBlock];
  const int tid = threadIdx.x;
  const int N = a.N, G = a.sh.G, nn = 2 * N - 1, S = a.S;
  int* const pre = a.pre + (size_t)blockIdx.x * (G + 1) * (N + 1);
  double* const slab = a.slab + (size_t)blockIdx.x * S * kBlock;
  const int chunk = (N + kBlock - 1) / kBlock;
  const int q0 = min(N, tid * chunk), q1 = min(N, q0 + chunk);
  for (int t = blockIdx.x; t < a.T; t += gridDim.x) {
    const int* leaf = a.leaf + (size_t)t * N;
    // 1. prefix counts, row by row: per-lane chunk counts, a serial scan of the kBlock partials, per-lane running sums
    for (int row = 0; row <= G; row++) {
      int cnt = 0;
      for (int q = q0; q < q1; q++) {
        const int x = leaf[q];
        cnt += (row < G) ? (a.sh.group[x] == row) : (int)a.sh.is_cond[x];
      }
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
        const int x = leaf[q];
        run += (row < G) ? (a.sh.group[x] == row) : (int)a.sh.is_cond[x];
      }
      __syncthreads();
    }
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

#define CC_TRY(expr)                                   \
  do {                                                 \
    hipError_t e_ = (expr);                            \
    if (e_ != hipSuccess) {                            \
      err_ = std::string(#expr) + ": " + hipGetErrorString(e_); \
      code_ = COLATE_EHIP;                             \
      return false;                                    \
    }                                                  \
  } while (0)

}  // namespace

struct CcDevice::Impl {
  int device = 0, N = 0, S = 0, F = 0, max_trees = 0, grid = 0;
  CcShared sh{};
  // run constants
  int *d_group = nullptr, *d_focal = nullptr;
  unsigned char* d_cond = nullptr;
  double* d_ages = nullptr;
  float *d_epochs = nullptr, *d_efocal = nullptr;
  int* d_pre = nullptr;
  double* d_slab = nullptr;
  // two chunk slots: pinned staging, device copies, per-tree results
  struct Slot {
    int T = 0;
    int *h_parent = nullptr, *h_lo = nullptr, *h_hi = nullptr, *h_leaf = nullptr;
    double* h_bl = nullptr;
    float* h_factor = nullptr;
    double* h_out = nullptr;
    std::vector<int> block;
    int *d_parent = nullptr, *d_lo = nullptr, *d_hi = nullptr, *d_leaf = nullptr;
    double* d_bl = nullptr;
    float* d_factor = nullptr;
    double* d_out = nullptr;
    hipEvent_t ev0 = nullptr, evk = nullptr, ev1 = nullptr;  // kernel start / kernel end / results copied back
    bool busy = false;
  } slot[2];
  int cur = 0;
  hipStream_t stream = nullptr;
  std::vector<std::vector<double>> acc;
};

bool CcDevice::fail(const char* what, int code) {
  err_ = what;
  code_ = code;
  return false;
}

CcDevice* CcDevice::create(int device, const CcRun& run, int max_trees, std::string& why) {
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
  CcDevice* d = new CcDevice();
  Impl* p = d->p_ = new Impl();
  p->device = device;
  p->N = run.N;
  p->S = run.slots();
  p->F = (int)run.focal.size();
  p->max_trees = std::max(1, max_trees);
  // the slabs take kBlock * S doubles per workgroup: at most ~2 GiB of them
  const size_t slab_bytes = (size_t)kBlock * p->S * sizeof(double);
  p->grid = (int)std::max<size_t>(1, std::min<size_t>({(size_t)kMaxGrid, (size_t)p->max_trees, ((size_t)2 << 30) / slab_bytes}));
  auto bad = [&](const std::string& w) {
    why = w;
    delete d;
    return (CcDevice*)nullptr;
  };
#define CC_MK(expr)                                                           \
  do {                                                                        \
    hipError_t e_ = (expr);                                                   \
    if (e_ != hipSuccess) return bad(std::string(#expr) + ": " + hipGetErrorString(e_)); \
  } while (0)
  CC_MK(hipSetDevice(device));
  CC_MK(hipStreamCreateWithFlags(&p->stream, hipStreamNonBlocking));
  const int N = run.N, nn = 2 * N - 1;
  CC_MK(hipMalloc(&p->d_group, sizeof(int) * N));
  CC_MK(hipMalloc(&p->d_cond, N));
  CC_MK(hipMalloc(&p->d_focal, sizeof(int) * std::max(1, p->F)));
  CC_MK(hipMalloc(&p->d_epochs, sizeof(float) * run.E()));
  CC_MK(hipMalloc(&p->d_efocal, sizeof(float) * run.EF()));
  CC_MK(hipMemcpy(p->d_group, run.group.data(), sizeof(int) * N, hipMemcpyHostToDevice));
  CC_MK(hipMemcpy(p->d_cond, run.is_cond.data(), N, hipMemcpyHostToDevice));
  if (p->F) CC_MK(hipMemcpy(p->d_focal, run.focal.data(), sizeof(int) * p->F, hipMemcpyHostToDevice));
  CC_MK(hipMemcpy(p->d_epochs, run.epochs.data(), sizeof(float) * run.E(), hipMemcpyHostToDevice));
  CC_MK(hipMemcpy(p->d_efocal, run.efocal.data(), sizeof(float) * run.EF(), hipMemcpyHostToDevice));
  if (!run.ages.empty()) {
    CC_MK(hipMalloc(&p->d_ages, sizeof(double) * N));
    CC_MK(hipMemcpy(p->d_ages, run.ages.data(), sizeof(double) * N, hipMemcpyHostToDevice));
  }
  CC_MK(hipMalloc(&p->d_pre, sizeof(int) * (size_t)p->grid * (run.G + 1) * (N + 1)));
  CC_MK(hipMalloc(&p->d_slab, slab_bytes * p->grid));
  const size_t T = p->max_trees;
  for (auto& s : p->slot) {
    CC_MK(hipHostMalloc(&s.h_parent, sizeof(int) * T * nn, hipHostMallocDefault));
    CC_MK(hipHostMalloc(&s.h_lo, sizeof(int) * T * nn, hipHostMallocDefault));
    CC_MK(hipHostMalloc(&s.h_hi, sizeof(int) * T * nn, hipHostMallocDefault));
    CC_MK(hipHostMalloc(&s.h_leaf, sizeof(int) * T * N, hipHostMallocDefault));
    CC_MK(hipHostMalloc(&s.h_bl, sizeof(double) * T * nn, hipHostMallocDefault));
    CC_MK(hipHostMalloc(&s.h_factor, sizeof(float) * T, hipHostMallocDefault));
    CC_MK(hipHostMalloc(&s.h_out, sizeof(double) * T * p->S, hipHostMallocDefault));
    CC_MK(hipMalloc(&s.d_parent, sizeof(int) * T * nn));
    CC_MK(hipMalloc(&s.d_lo, sizeof(int) * T * nn));
    CC_MK(hipMalloc(&s.d_hi, sizeof(int) * T * nn));
    CC_MK(hipMalloc(&s.d_leaf, sizeof(int) * T * N));
    CC_MK(hipMalloc(&s.d_bl, sizeof(double) * T * nn));
    CC_MK(hipMalloc(&s.d_factor, sizeof(float) * T));
    CC_MK(hipMalloc(&s.d_out, sizeof(double) * T * p->S));
    CC_MK(hipEventCreate(&s.ev0));
    CC_MK(hipEventCreate(&s.evk));
    CC_MK(hipEventCreate(&s.ev1));
  }
#undef CC_MK
  p->sh.N = N;
  p->sh.G = run.G;
  p->sh.E = run.E();
  p->sh.EF = run.EF();
  p->sh.group = p->d_group;
  p->sh.is_cond = p->d_cond;
  p->sh.cond_empty = run.cond_empty ? 1 : 0;
  p->sh.ages = p->d_ages;
  p->sh.epochs = p->d_epochs;
  p->sh.efocal = p->d_efocal;
  return d;
}

CcDevice::~CcDevice() {
  if (!p_) return;
  Impl* p = p_;
  if (p->stream) (void)hipStreamSynchronize(p->stream);
  for (auto& s : p->slot) {
    for (void* h : {(void*)s.h_parent, (void*)s.h_lo, (void*)s.h_hi, (void*)s.h_leaf, (void*)s.h_bl, (void*)s.h_factor, (void*)s.h_out})
      if (h) (void)hipHostFree(h);
    for (void* q : {(void*)s.d_parent, (void*)s.d_lo, (void*)s.d_hi, (void*)s.d_leaf, (void*)s.d_bl, (void*)s.d_factor, (void*)s.d_out})
      if (q) (void)hipFree(q);
    if (s.ev0) (void)hipEventDestroy(s.ev0);
    if (s.evk) (void)hipEventDestroy(s.evk);
    if (s.ev1) (void)hipEventDestroy(s.ev1);
  }
  for (void* q : {(void*)p->d_group, (void*)p->d_cond, (void*)p->d_focal, (void*)p->d_ages, (void*)p->d_epochs, (void*)p->d_efocal,
                  (void*)p->d_pre, (void*)p->d_slab})
    if (q) (void)hipFree(q);
  if (p->stream) (void)hipStreamDestroy(p->stream);
  delete p;
}

// waits for a slot's launch and adds its trees into their blocks, in tree order
bool CcDevice::drain(int k) {
  Impl::Slot& s = p_->slot[k];
  if (!s.busy) return true;
  CC_TRY(hipEventSynchronize(s.ev1));
  float ms = 0.f;
  if (hipEventElapsedTime(&ms, s.ev0, s.evk) == hipSuccess) gpu_s_ += ms * 1e-3;
  const int S = p_->S;
  for (int t = 0; t < s.T; t++) {
    const int b = s.block[t];
    if ((int)p_->acc.size() <= b) p_->acc.resize(b + 1);
    std::vector<double>& dst = p_->acc[b];
    if (dst.empty()) dst.assign(S, 0.0);
    const double* src = s.h_out + (size_t)t * S;
    for (int c = 0; c < S; c++) dst[c] += src[c];
  }
  s.busy = false;
  return true;
}

bool CcDevice::submit(const CcChunk& c) {
  Impl* p = p_;
  if (c.T == 0) return true;
  if (c.T > p->max_trees || c.N != p->N) return fail("condcoal: chunk larger than the device buffers", COLATE_EINVAL);
  const int k = p->cur;
  p->cur ^= 1;
  if (!drain(k)) return false;
  Impl::Slot& s = p->slot[k];
  const int N = p->N, nn = 2 * N - 1;
  const size_t T = c.T;
  std::memcpy(s.h_parent, c.parent.data(), sizeof(int) * T * nn);
  std::memcpy(s.h_lo, c.lo.data(), sizeof(int) * T * nn);
  std::memcpy(s.h_hi, c.hi.data(), sizeof(int) * T * nn);
  std::memcpy(s.h_leaf, c.leaf.data(), sizeof(int) * T * N);
  std::memcpy(s.h_bl, c.bl.data(), sizeof(double) * T * nn);
  std::memcpy(s.h_factor, c.factor.data(), sizeof(float) * T);
  s.block = c.block;
  s.T = c.T;
  CC_TRY(hipSetDevice(p->device));
  CC_TRY(hipMemcpyAsync(s.d_parent, s.h_parent, sizeof(int) * T * nn, hipMemcpyHostToDevice, p->stream));
  CC_TRY(hipMemcpyAsync(s.d_lo, s.h_lo, sizeof(int) * T * nn, hipMemcpyHostToDevice, p->stream));
  CC_TRY(hipMemcpyAsync(s.d_hi, s.h_hi, sizeof(int) * T * nn, hipMemcpyHostToDevice, p->stream));
  CC_TRY(hipMemcpyAsync(s.d_leaf, s.h_leaf, sizeof(int) * T * N, hipMemcpyHostToDevice, p->stream));
  CC_TRY(hipMemcpyAsync(s.d_bl, s.h_bl, sizeof(double) * T * nn, hipMemcpyHostToDevice, p->stream));
  CC_TRY(hipMemcpyAsync(s.d_factor, s.h_factor, sizeof(float) * T, hipMemcpyHostToDevice, p->stream));
  KernelArgs a;
  a.T = c.T;
  a.N = N;
  a.F = p->F;
  a.S = p->S;
  a.parent = s.d_parent;
  a.lo = s.d_lo;
  a.hi = s.d_hi;
  a.leaf = s.d_leaf;
  a.bl = s.d_bl;
  a.factor = s.d_factor;
  a.focal = p->d_focal;
  a.sh = p->sh;
  a.pre = p->d_pre;
  a.slab = p->d_slab;
  a.out = s.d_out;
  const int grid = std::min(p->grid, c.T);
  CC_TRY(hipEventRecord(s.ev0, p->stream));
  hipLaunchKernelGGL(condcoal_kernel, dim3(grid), dim3(kBlock), 0, p->stream, a);
  CC_TRY(hipGetLastError());
  CC_TRY(hipEventRecord(s.evk, p->stream));
  CC_TRY(hipMemcpyAsync(s.h_out, s.d_out, sizeof(double) * T * p->S, hipMemcpyDeviceToHost, p->stream));
  CC_TRY(hipEventRecord(s.ev1, p->stream));
  s.busy = true;
  return true;
}

bool CcDevice::finish(std::vector<std::vector<double>>& acc) {
  if (!drain(p_->cur) || !drain(p_->cur ^ 1)) return false;
  acc = std::move(p_->acc);
  p_->acc.clear();
  return true;
}

}  // namespace colate_cc
