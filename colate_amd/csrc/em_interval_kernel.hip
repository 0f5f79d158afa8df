// colate_amd/csrc/em_interval_kernel.hip -- coal_EM::EM_shared / EM_notshared for R calls (kind, age_begin, age_end)
// against one (epochs[E], rates[E]) on gfx950: the functions of em_interval.hpp with the epochs of a call strided over
// the 64 lanes of one wavefront.
//
// One wavefront per call, WAVES calls per workgroup.  A_ep / B_ep (get_AB) are computed once per workgroup into LDS.
// The call itself (its phases and barriers) is wave_call() of em_interval_wave.hpp, which the EM fit shares: the device
// equals the host twin (em_interval::call<EmMath>) bit for bit.  A wave whose call index is beyond R works on the last
// call and stores nothing.
#include <hip/hip_runtime.h>

#include "em_interval_wave.hpp"
#include "em_kernels.h"

namespace {

using namespace em_interval;

template <int WAVES>
__global__ __launch_bounds__(WAVES * 64) void em_interval_kernel(int R, int E, const int* __restrict__ kinds,
                                                                 const double* __restrict__ age_begin,
                                                                 const double* __restrict__ age_end,
                                                                 const double* __restrict__ epochs,
                                                                 const double* __restrict__ rates,
                                                                 double* __restrict__ out_num, double* __restrict__ out_den,
                                                                 double* __restrict__ out_logl, int* __restrict__ out_flags) {
  extern __shared__ double smem[];
  double* tab = smem;
  double* ep = tab + em::kExpTableDoubles;
  double* rt = ep + E;
  double* A = rt + E;
  double* B = A + E;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const WaveLds w = wave_lds(B + E, E, wave);

  // ---- per workgroup: the grid, the exp table, A_ep / B_ep
  for (int i = tid; i < em::kExpTableDoubles; i += WAVES * 64) tab[i] = em::kExpTableDevice[i];
  for (int e = tid; e < E; e += WAVES * 64) ep[e] = epochs[e], rt[e] = rates[e];
  __syncthreads();
  const EmMath m{tab};
  double* cum_ab = B + E;  // (wave 0's cse: free until the barrier after ab_at)
  if (tid == 0) ab_prefix(E, ep, rt, cum_ab);
  __syncthreads();
  for (int e = tid; e < E; e += WAVES * 64) ab_at(m, E, ep, rt, cum_ab, e, A, B);
  __syncthreads();

  // ---- per wave: one call
  const int r_raw = blockIdx.x * WAVES + wave;
  const bool valid = r_raw < R;
  const int r = valid ? r_raw : R - 1;
  const View v{E, ep, rt, A, B};
  double logl;
  const int flags = wave_call(m, v, kinds[r], age_begin[r], age_end[r], true, lane, w, &logl);
  if (!valid) return;
  for (int e = lane; e < E; e += 64) out_num[(size_t)r * E + e] = w.num[e], out_den[(size_t)r * E + e] = w.den[e];
  if (lane == 0) {
    out_logl[r] = logl;
    out_flags[r] = flags;
  }
}

// The E-step over the calls (coal.cpp:3704-3733 with weights for counts): num_acc[e] = sum_r w[r] num[r][e] and so on,
// rows in ascending order, one thread per epoch and one for the log-likelihood: no atomics, one fixed order.
__global__ __launch_bounds__(256) void em_interval_accumulate_kernel(int R, int E, const double* __restrict__ weights,
                                                                     const double* __restrict__ num,
                                                                     const double* __restrict__ den,
                                                                     const double* __restrict__ logl,
                                                                     double* __restrict__ num_acc,
                                                                     double* __restrict__ den_acc, double* __restrict__ ll) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t < E) {
    double n = 0.0, d = 0.0;
    for (int r = 0; r < R; r++) {
      const double w = weights[r];
      if (w > 0) {  // (the reference visits bins with a count only)
        n += w * num[(size_t)r * E + t];
        d += w * den[(size_t)r * E + t];
      }
    }
    num_acc[t] = n, den_acc[t] = d;
  } else if (t == E) {
    double s = 0.0;
    for (int r = 0; r < R; r++) {
      const double w = weights[r];
      if (w > 0) s += w * logl[r];
    }
    *ll = s;
  }
}

}  // namespace

hipError_t colate_em_interval_launch(int R, int E, const int* kinds, const double* age_begin, const double* age_end,
                                     const double* epochs, const double* rates, const double* weights, double* out_num,
                                     double* out_den, double* out_logl, int* out_flags, double* out_num_acc,
                                     double* out_den_acc, double* out_ll, hipStream_t stream) {
  if (R <= 0) return hipSuccess;
  if (E < 1 || E > COLATE_EM_MAX_E) return hipErrorInvalidValue;
  if (E <= 256) {  // four calls per workgroup: 34 KiB of LDS at E = 256
    constexpr int W = 4;
    em_interval_kernel<W><<<(R + W - 1) / W, W * 64, lds_doubles(E, W) * sizeof(double), stream>>>(
        R, E, kinds, age_begin, age_end, epochs, rates, out_num, out_den, out_logl, out_flags);
  } else {  // one call per workgroup: 57 KiB at E = 1024
    em_interval_kernel<1><<<R, 64, lds_doubles(E, 1) * sizeof(double), stream>>>(R, E, kinds, age_begin, age_end, epochs,
                                                                                  rates, out_num, out_den, out_logl, out_flags);
  }
  if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
  if (weights) {
    em_interval_accumulate_kernel<<<(E + 1 + 255) / 256, 256, 0, stream>>>(R, E, weights, out_num, out_den, out_logl,
                                                                          out_num_acc, out_den_acc, out_ll);
    return hipGetLastError();
  }
  return hipSuccess;
}
