// colate_amd/csrc/coalrate_tree_kernel.hip -- the per-tree sort of `CoalRate --mode tree` on the device (coalrate_tree.h:
// the walk and the one summation order, shared with the host twin).  Per chunk of calls, two launches on one stream:
//   * crt_sort: a call's lanes build the 64-bit keys (time bits above the label) of its 2N-1 nodes, padded with ~0 to a
//     power of two P, and sort them by a bitonic network -- in LDS while P <= kLdsKeys (N <= 8192: 128 KiB of the 160 KiB
//     a workgroup may ask for), in device memory beyond that (the same code over another pointer; a workgroup's own
//     writes are ordered by its barriers).  Then an inclusive scan of +1 / -1 over the sorted order (per-lane stretches, a
//     serial scan of the stretch totals), the scan value of every tie group's last position carried back over the group
//     (num_lins), both packed into the key's low word in place of the label; the epochs' first positions by bisection;
//     and per epoch the 64 partial sums of coalrate_tree.h, 64 lanes to an epoch, added in order by one lane.
//     Small trees share a workgroup (lanes per call = P / 2, at least 4) once a chunk has more calls than the chip has
//     wave slots.  Out: count / den [call][E].
//   * crt_fold: one lane per epoch adds the calls' addends into their blocks in call order; the per-block sums stay on the
//     device until finish().
// No atomics: every output word has one writer.  The walker around the two launches is coalrate_device.hpp's.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include "coalrate_device.hpp"
#include "coalrate_tree.h"

namespace colate_crt {

namespace {

using colate::Staged;
using colate_cr::kLdsBytes;
using colate_cr::kMaxLanes;

struct SortArgs {
  int T, N, P, E;
  int cpw, lpc;                // calls per workgroup, lanes per call
  const float* t;              // [T][2N-1]
  const double* epochs;        // [E]
  const double* w;             // [T]
  unsigned long long* gkeys;   // [T][P] (the device-memory path)
  int* count;                  // [T][E]
  double* den;                 // [T][E]
};

// per-call LDS beside the keys: kPartials-or-lpc partial sums and counts, lpc stretch totals, E first positions
__host__ __device__ inline int crt_round_lanes(int lpc) { return lpc < kPartials ? kPartials : lpc; }

struct KeyRead {
  const unsigned long long* p;
  __device__ unsigned long long operator()(int k) const { return p[k]; }
};
struct TimeRead {
  const unsigned* w;  // the keys as 32-bit words: the time of position k is word 2k+1
  __device__ double operator()(int k) const { return (double)__uint_as_float(w[2 * k + 1]); }
};

template <bool kLds>
__global__ void __launch_bounds__(kMaxLanes) crt_sort(SortArgs a) {
  extern __shared__ unsigned long long s_mem[];
  const int slot = threadIdx.x / a.lpc, lane = threadIdx.x % a.lpc;
  const int k = blockIdx.x * a.cpw + slot;
  const bool active = slot < a.cpw && k < a.T;
  const int N = a.N, nn = 2 * N - 1, P = a.P, E = a.E, lpc = a.lpc, rl = crt_round_lanes(lpc);
  // LDS: (kLds) the keys of every slot; the partial sums of every slot; then the ints: partial counts, stretch totals,
  // first positions
  unsigned long long* keys = kLds ? s_mem + (size_t)slot * P : a.gkeys + (size_t)(active ? k : 0) * P;
  double* psum = reinterpret_cast<double*>(s_mem + (kLds ? (size_t)a.cpw * P : 0)) + (size_t)slot * rl;
  int* ints = reinterpret_cast<int*>(s_mem + (kLds ? (size_t)a.cpw * P : 0) + (size_t)a.cpw * rl);
  int* pcnt = ints + (size_t)slot * rl;
  int* part = ints + (size_t)a.cpw * rl + (size_t)slot * lpc;
  int* first = ints + (size_t)a.cpw * (rl + lpc) + (size_t)slot * E;
  unsigned* words = reinterpret_cast<unsigned*>(keys);  // low word of position q at 2q, high word at 2q+1

  if (active) {
    const float* t = a.t + (size_t)k * nn;
    for (int v = lane; v < P; v += lpc) keys[v] = v < nn ? crt_key(t[v], v) : ~0ull;
  }
  __syncthreads();
  // the bitonic network: P / 2 compare-exchanges per step
  for (int kk = 2; kk <= P; kk <<= 1)
    for (int j = kk >> 1; j > 0; j >>= 1) {
      if (active)
        for (int idx = lane; idx < P / 2; idx += lpc) {
          const int i = 2 * idx - (idx & (j - 1)), l = i + j;
          const unsigned long long x = keys[i], y = keys[l];
          if ((x > y) == ((i & kk) == 0)) {
            keys[i] = y;
            keys[l] = x;
          }
        }
      __syncthreads();
    }
  // the scan of +1 (label < N) / -1 over the sorted order; a lane's stretch has an odd length (LDS banks)
  const int len = ((nn + lpc - 1) / lpc) | 1, q0 = min(nn, lane * len), q1 = min(nn, q0 + len);
  if (active) {
    int d = 0;
    for (int q = q0; q < q1; q++) d += ((int)words[2 * q] < N) ? 1 : -1;
    part[lane] = d;
  }
  __syncthreads();
  if (active && lane == 0) {
    int run = 0;
    for (int l = 0; l < lpc; l++) {
      const int c = part[l];
      part[l] = run;
      run += c;
    }
  }
  __syncthreads();
  if (active) {
    int run = part[lane];
    for (int q = q0; q < q1; q++) {
      const bool internal = (int)words[2 * q] >= N;
      run += internal ? -1 : 1;
      words[2 * q] = crt_pack(run, internal);
    }
  }
  __syncthreads();
  // num_lins: the scan value of the last position of every tie group.  A group that runs on beyond this lane's stretch
  // ends where bisection over the times finds it; that value is read before any lane overwrites one.
  int carried = 0;
  bool carry = false;
  if (active && q1 > q0 && q1 < nn && words[2 * q1 + 1] == words[2 * (q1 - 1) + 1]) {
    const unsigned hi_word = words[2 * (q1 - 1) + 1];
    int lo = q1, hi = nn;  // the first position in [q1, nn] whose time is above hi_word
    while (lo < hi) {
      const int mid = (lo + hi) / 2;
      if (words[2 * mid + 1] <= hi_word) lo = mid + 1;
      else hi = mid;
    }
    carried = (int)words[2 * (lo - 1)] >> 1;
    carry = true;
  }
  __syncthreads();
  if (active) {
    int cur = carried;
    for (int q = q1 - 1; q >= q0; q--) {
      const unsigned low = words[2 * q];
      const bool ends = (q == q1 - 1) ? !carry : words[2 * q + 1] != words[2 * q + 3];
      if (ends) cur = (int)low >> 1;
      words[2 * q] = crt_pack(cur, low & 1u);
    }
  }
  __syncthreads();
  const TimeRead time{words};
  if (active)
    for (int e = lane; e < E; e += lpc) first[e] = e ? crt_first(time, nn, a.epochs[e]) : 1;
  __syncthreads();
  // the epoch sums: `per` epochs at a time, 64 partial sums each
  const int per = lpc < kPartials ? 1 : lpc / kPartials, jstep = lpc < kPartials ? lpc : kPartials;
  const int sub = lane / kPartials, jl = lane % kPartials;
  const double w = active ? a.w[k] : 0.0;
  const KeyRead rd{keys};
  for (int e0 = 0; e0 + 1 < E; e0 += per) {
    const int e = e0 + sub;
    const bool mine = active && e + 1 < E;
    if (mine)
      for (int j = jl; j < kPartials; j += jstep) {
        int c = 0;
        psum[sub * kPartials + j] = crt_partial(rd, nn, a.epochs, e, first[e], first[e + 1], j, w, c);
        pcnt[sub * kPartials + j] = c;
      }
    __syncthreads();
    if (mine && jl == 0) {
      double s = 0.0;
      int c = 0;
      for (int j = 0; j < kPartials; j++) {
        s += psum[sub * kPartials + j];
        c += pcnt[sub * kPartials + j];
      }
      a.den[(size_t)k * E + e] = s;
      a.count[(size_t)k * E + e] = c;
    }
    __syncthreads();
  }
  if (active && lane == 0) {  // nothing reaches the last cell
    a.den[(size_t)k * E + E - 1] = 0.0;
    a.count[(size_t)k * E + E - 1] = 0;
  }
}

struct FoldArgs {
  int T, E;
  const int* count;
  const double* den;
  const double* w;
  const int* block;
  double* num;  // [blocks][E]
  double* dsum;
};

__global__ void __launch_bounds__(kMaxLanes) crt_fold(FoldArgs a) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= a.E) return;
  int cur = -1;
  double num = 0.0, den = 0.0;
  for (int k = 0; k < a.T; k++) {
    const int b = a.block[k];
    if (b != cur) {
      if (cur >= 0) {
        a.num[(size_t)cur * a.E + e] = num;
        a.dsum[(size_t)cur * a.E + e] = den;
      }
      cur = b;
      num = a.num[(size_t)cur * a.E + e];
      den = a.dsum[(size_t)cur * a.E + e];
    }
    num += (double)a.count[(size_t)k * a.E + e] * (a.w[k] / 1e9);
    den += a.den[(size_t)k * a.E + e];
  }
  if (cur >= 0) {
    a.num[(size_t)cur * a.E + e] = num;
    a.dsum[(size_t)cur * a.E + e] = den;
  }
}

struct CrtArrays {  // the calls of one launch
  Staged<float> t;
  Staged<double> w;
  Staged<int> block;
};

class DeviceWalker final : public colate_cr::BlockSumDeviceWalker<CrtChunk, CrtArrays> {
 public:
  DeviceWalker() : BlockSumDeviceWalker("coalrate tree") {}

  bool open(int device, int N, const std::vector<double>& epochs, int max_calls) {
    if (!open_device(device)) return false;
    E_ = (int)epochs.size(), P_ = padded_keys(N);
    if (E_ > kMaxDeviceEpochs)
      return fail(std::to_string(E_) + " epochs are more than the kernel keeps in LDS (" + std::to_string(kMaxDeviceEpochs) + ")",
                  COLATE_ELIMIT);
    lpc_ = std::min(kMaxLanes, std::max(4, P_ / 2));
    lds_keys_ = P_ <= kLdsKeys;
    const int rl = crt_round_lanes(lpc_);
    call_lds_ = (lds_keys_ ? sizeof(unsigned long long) * P_ : 0) + (sizeof(double) + sizeof(int)) * rl +
                sizeof(int) * ((size_t)lpc_ + E_);
    cpw_cap_ = (int)std::max<size_t>(1, std::min<size_t>(kMaxLanes / lpc_, (kLdsBytes - 8) / call_lds_));
    if (!open_sums(N, max_calls, E_)) return false;
    WALKER_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&crt_sort<true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsBytes));
    WALKER_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&crt_sort<false>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsBytes));
    if (!upload(epochs_, epochs)) return false;
    const size_t T = max_calls_, nn = 2 * (size_t)N_ - 1;
    for (Slot& s : slot_)
      if (!make(s.t, T * nn) || !make(s.w, T) || !make(s.block, T)) return false;
    // the kernels' intermediate results are used within the stream's order: one copy serves both slots
    WALKER_TRY(buf_.device(count_, T * E_));
    WALKER_TRY(buf_.device(cden_, T * E_));
    if (!lds_keys_) WALKER_TRY(buf_.device(gkeys_, T * P_));
    return true;
  }

 private:
  bool stage(Slot& s, const CrtChunk& c, int t0, int T) override {
    const size_t nn = 2 * (size_t)N_ - 1;
    return send(s.t, c.t.data() + t0 * nn, T * nn) && send(s.w, c.w.data() + t0, T) && send(s.block, c.block.data() + t0, T);
  }
  bool launch(Slot& s, int T) override {
    const Shape sh = launch_shape(T);
    SortArgs sa{T, N_, P_, E_, sh.cpw, lpc_, s.t.d, epochs_, s.w.d, gkeys_, count_, cden_};
    const size_t lds = (call_lds_ * sh.cpw + 7) / 8 * 8;
    if (lds_keys_) hipLaunchKernelGGL(crt_sort<true>, dim3(sh.grid), dim3(sh.lanes), lds, stream_, sa);
    else hipLaunchKernelGGL(crt_sort<false>, dim3(sh.grid), dim3(sh.lanes), lds, stream_, sa);
    WALKER_TRY(hipGetLastError());
    colate_cr::launch_stats(colate_cr::kLaunchTree).note(sh.cpw, lpc_, lds_keys_);
    FoldArgs fa{T, E_, count_, cden_, s.w.d, s.block.d, num_, den_};
    hipLaunchKernelGGL(crt_fold, dim3((E_ + 63) / 64), dim3(64), 0, stream_, fa);
    WALKER_TRY(hipGetLastError());
    return true;
  }

  int E_ = 0, P_ = 0;
  bool lds_keys_ = true;
  size_t call_lds_ = 0;
  double* epochs_ = nullptr;
  int* count_ = nullptr;
  double* cden_ = nullptr;
  unsigned long long* gkeys_ = nullptr;
};

}  // namespace

std::unique_ptr<CoalTreeWalker> make_device_walker(int device, int N, const std::vector<double>& epochs, int max_calls,
                                                   std::string& why, int* code) {
  auto w = std::make_unique<DeviceWalker>();
  if (!w->open(device, N, epochs, max_calls)) {
    why = w->error();
    if (code) *code = w->error_code();
    return nullptr;
  }
  return w;
}

}  // namespace colate_crt
