// colate_amd/csrc/coalrate_tree.h -- `CoalRate --mode tree` inside libcolate_amd.so (coal_tree::populate,
// include/coal/coal_tree.cpp:100-178): what the host side (coalrate_tree.cpp: preparation of the calls, host twin, C
// ABI; coalrate.cpp: the driver) and the device side (coalrate_tree_kernel.hip) share.  DESIGN.md ("CoalRate --mode tree") has the derivation.
//
// One call = one tree with a weight w and a block.  Its 2N-1 node times (float, Tree::GetCoordinates) are sorted by
// (time, label): a 64-bit key, the time's bit pattern above the label, in unsigned order.  Over the sorted positions
// k = 0 .. 2N-2, num_lins[k] is the running count (+1 for a label < N, -1 otherwise) at the last position that ties with
// k.  populate then walks the positions k = 1 .. 2N-2 against the epoch boundaries; restated per epoch e (cells
// 0 .. E-2; nothing reaches cell E-1) with first[e] = 1 + #{k >= 1 : t_k <= epochs[e]} (first[0] = 1):
//   * the node pieces i = 0 .. m-1, m = first[e+1] - first[e], k = first[e] + i:
//       w * L * (L - 1) / 2.0 * (upper - lower) / 1e9,  L = num_lins[k-1], upper = (double)t_k,
//       lower = (double)t_{k-1}, or epochs[e] for i = 0 (so the first piece of a tree starts at epochs[0] = 0 even when
//       every sample is ancient, as the reference's running lower age does);
//   * the closing piece i = m while nodes remain (first[e+1] < 2N-1): L = num_lins[first[e+1]-1], upper = epochs[e+1],
//     lower = the last node's time, or epochs[e] for m = 0;
//   * the numerator's count: the positions of the epoch whose label is >= N.
// THE ONE SUMMATION ORDER, for the kernel and the host twin alike:
//   * per (call, epoch) the pieces go into kPartials = 64 partial sums, piece i into partial i % 64, each partial adding
//     its pieces in ascending i from 0.0; the epoch's sum adds the partials 0 .. 63 in ascending order from 0.0;
//   * per (block, epoch) denom += that sum and num += (double)count * (w / 1e9), over the calls in input order.
// Counts are integers and are combined in any order.  No float atomics anywhere.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "coalrate.h"

namespace colate_crt {

using colate_cc::kMaxHaplotypes;
using colate_cr::CrSums;  // per-block sums num / den [block][E]

constexpr int kPartials = 64;     // partial sums per (call, epoch)
constexpr int kLdsKeys = 16384;   // keys (2N-1 padded to a power of two) up to which the device sorts in LDS: N <= 8192
constexpr int kMaxDeviceEpochs = 1024;  // epochs whose starts the kernel keeps in LDS

CR_HD unsigned crt_float_bits(float t) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __float_as_uint(t);
#else
  unsigned u;
  std::memcpy(&u, &t, sizeof u);
  return u;
#endif
}
CR_HD float crt_bits_float(unsigned u) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __uint_as_float(u);
#else
  float t;
  std::memcpy(&t, &u, sizeof t);
  return t;
#endif
}

// The key of a node before the sort; times are non-negative (+0 included), so unsigned order is (time, label) order.
CR_HD unsigned long long crt_key(float t, int label) { return ((unsigned long long)crt_float_bits(t) << 32) | (unsigned)label; }
// After the sort and the scan the low word of position k holds num_lins[k] and whether the node is internal.
CR_HD unsigned crt_pack(int lins, bool internal) { return ((unsigned)lins << 1) | (internal ? 1u : 0u); }
CR_HD double crt_time(unsigned long long key) { return (double)crt_bits_float((unsigned)(key >> 32)); }
CR_HD int crt_lins(unsigned long long key) { return (int)(unsigned)key >> 1; }

// coal_tree.cpp:160 / 168, left to right in double
CR_HD double crt_piece(double w, int L, double upper, double lower) { return w * L * (L - 1) / 2.0 * (upper - lower) / 1e9; }

// Partial j of epoch e of one call: key(k) is the packed key of sorted position k, nn = 2N-1, [f0, f1) = first[e],
// first[e+1].  Adds the internal nodes among its pieces to `internal`.
template <class Key>
CR_HD double crt_partial(Key key, int nn, const double* epochs, int e, int f0, int f1, int j, double w, int& internal) {
  const int m = f1 - f0, pieces = m + (f1 < nn ? 1 : 0);
  double s = 0.0;
  for (int i = j; i < pieces; i += kPartials) {
    if (i < m) {
      const unsigned long long prev = key(f0 + i - 1), cur = key(f0 + i);
      internal += (int)(cur & 1u);
      s += crt_piece(w, crt_lins(prev), crt_time(cur), i ? crt_time(prev) : epochs[e]);
    } else {
      const unsigned long long prev = key(f1 - 1);
      s += crt_piece(w, crt_lins(prev), epochs[e + 1], m ? crt_time(prev) : epochs[e]);
    }
  }
  return s;
}

// first[e] of the header comment, by bisection over the sorted times: time(k) for k in [1, nn).
template <class Time>
CR_HD int crt_first(Time time, int nn, double boundary) {
  int lo = 1, hi = nn;  // the first k in [1, nn] with time(k) > boundary
  while (lo < hi) {
    const int mid = (lo + hi) / 2;
    if (time(mid) <= boundary) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// A chunk of prepared calls: the node times, back to back.
struct CrtChunk {
  int N = 0, T = 0;
  std::vector<float> t;  // [T][2N-1]
  std::vector<double> w;
  std::vector<int> block;
  void clear() {
    T = 0;
    t.clear(), w.clear(), block.clear();
  }
  int append(int n) {  // room for one more call; returns its index
    N = n;
    t.resize(t.size() + (2 * (size_t)n - 1));
    w.push_back(0.0);
    block.push_back(0);
    return T++;
  }
};

// The node times of a raw tree (Relate labelling) as Tree::GetCoordinates dates them (float; leaves at 0 or at their
// sample age).  False with a message for a malformed tree (colate_cc::prepare_tree; a negative or NaN time; a node younger
// than a child) or a node older than the last epoch boundary.  ages: [N] or null.
bool prepare_times(int N, const double* ages, const std::vector<double>& epochs, const int* parent, const double* bl, float* t,
                   std::string& err);

// chunks in, per-block sums [block][E] out, the same bits from the host twin and the device
using CoalTreeWalker = colate_cr::BlockSumWalker<CrtChunk>;

std::unique_ptr<CoalTreeWalker> make_host_walker(int N, const std::vector<double>& epochs);
// Null, the reason in `why` and its COLATE_E code in *code, when there is no device or the run does not fit it (device -1:
// the calling thread's).
std::unique_ptr<CoalTreeWalker> make_device_walker(int device, int N, const std::vector<double>& epochs, int max_calls,
                                                   std::string& why, int* code = nullptr);
// Calls per chunk: the most that fit 4M node times and 256 MiB of device memory, or COLATE_COALRATE_CHUNK_TREES where that
// is set and smaller.
int chunk_calls_for(int N, int E);
// 2N-1 padded to a power of two: the keys of a call's sort
inline int padded_keys(int N) {
  int P = 4;
  while (P < 2 * N - 1) P *= 2;
  return P;
}

}  // namespace colate_crt
