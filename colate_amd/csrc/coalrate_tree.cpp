// colate_amd/csrc/coalrate_tree.cpp -- `CoalRate --mode tree` (coal_tree::populate, include/coal/coal_tree.cpp:100-178):
//   * the preparation of a call (a tree checked and dated as Tree::GetCoordinates dates it);
//   * the host twin of the device's sort, scan and epoch sums (coalrate_tree.h: the walk and the one summation order);
//   * the C ABI over raw trees (colate_coalrate_tree_accumulate[_host]).
// The driver is coalrate.cpp's run_tree; the C ABI body runs on coalrate.h's BlockAccumulate.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <limits>

#include "coalrate_tree.h"
#include "colate_amd.h"
#include "colate_internal.h"

namespace colate_crt {

bool prepare_times(int N, const double* ages, const std::vector<double>& epochs, const int* parent, const double* bl, float* t,
                   std::string& err) {
  const int nn = 2 * N - 1;
  std::vector<int> lo(nn), hi(nn), leaf(N);
  if (!colate_cc::prepare_tree(N, parent, lo.data(), hi.data(), leaf.data(), err)) return false;
  // children before parents: coordinates[n] = max(coordinates[child] + branch_length) as a float (anc.cpp:280-308)
  std::vector<double> best(nn, -std::numeric_limits<double>::infinity());
  std::vector<int> pending(nn, 2), queue;
  queue.reserve(nn);
  for (int i = 0; i < N; i++) {
    t[i] = ages ? (float)ages[i] : 0.f;
    queue.push_back(i);
  }
  for (size_t h = 0; h < queue.size(); h++) {
    const int x = queue[h], p = parent[x];
    if (p < 0) continue;
    best[p] = std::max(best[p], (double)t[x] + bl[x]);
    if (--pending[p] == 0) {
      t[p] = (float)best[p];
      queue.push_back(p);
    }
  }
  const double last = epochs.back();
  for (int v = 0; v < nn; v++) {
    if (!(t[v] >= 0.f)) {
      err = (v < N ? "sample " : "node ") + std::to_string(v) + " has time " + std::to_string(t[v]);
      return false;
    }
    if (t[v] == 0.f) t[v] = 0.f;  // (+0: the keys order by bit pattern)
    if ((double)t[v] > last) {
      err = "node " + std::to_string(v) + " (time " + std::to_string(t[v]) + ") is older than the last epoch boundary " +
            std::to_string(last);
      return false;
    }
    if (parent[v] >= 0 && t[parent[v]] < t[v]) {
      err = "node " + std::to_string(parent[v]) + " is younger than its child " + std::to_string(v);
      return false;
    }
  }
  return true;
}

int chunk_calls_for(int N, int E) {
  const size_t nn = 2 * (size_t)N - 1;
  const size_t bytes = sizeof(float) * nn + (sizeof(int) + sizeof(double)) * E + sizeof(double) + sizeof(int) +
                       (padded_keys(N) > kLdsKeys ? sizeof(unsigned long long) * padded_keys(N) : 0);
  int calls = (int)std::max<size_t>(1, std::min<size_t>((4u << 20) / nn, ((size_t)256 << 20) / bytes));
  if (const char* e = std::getenv("COLATE_COALRATE_CHUNK_TREES")) {
    const int k = std::atoi(e);
    if (k >= 1) calls = std::min(calls, k);
  }
  return calls;
}

namespace {

class HostWalker final : public CoalTreeWalker {
 public:
  HostWalker(int N, const std::vector<double>& epochs) : N_(N), epochs_(epochs) {}
  bool submit(const CrtChunk& c) override {
    const int N = N_, nn = 2 * N - 1, E = (int)epochs_.size();
    std::vector<unsigned long long> key(nn);
    std::vector<int> scan(nn);
    for (int k = 0; k < c.T; k++) {
      const float* t = c.t.data() + (size_t)k * nn;
      for (int v = 0; v < nn; v++) key[v] = crt_key(t[v], v);
      std::sort(key.begin(), key.end());
      int run = 0;
      for (int q = 0; q < nn; q++) scan[q] = run += ((int)(unsigned)key[q] < N) ? 1 : -1;
      int cur = 0;
      for (int q = nn - 1; q >= 0; q--) {  // num_lins: the scan at the last position of every tie group
        if (q == nn - 1 || (key[q] >> 32) != (key[q + 1] >> 32)) cur = scan[q];
        key[q] = (key[q] & 0xffffffff00000000ull) | crt_pack(cur, (int)(unsigned)key[q] >= N);
      }
      const int b = c.block[k];
      if (b >= sums_.blocks) {
        sums_.blocks = b + 1;
        sums_.num.resize((size_t)sums_.blocks * E, 0.0);
        sums_.den.resize((size_t)sums_.blocks * E, 0.0);
      }
      const auto rd = [&](int q) { return key[q]; };
      const auto time = [&](int q) { return crt_time(key[q]); };
      const double w = c.w[k];
      int f0 = 1;
      for (int e = 0; e + 1 < E; e++) {
        const int f1 = crt_first(time, nn, epochs_[e + 1]);
        int count = 0;
        double s = 0.0;
        for (int j = 0; j < kPartials; j++) s += crt_partial(rd, nn, epochs_.data(), e, f0, f1, j, w, count);
        sums_.num[(size_t)b * E + e] += (double)count * (w / 1e9);
        sums_.den[(size_t)b * E + e] += s;
        f0 = f1;
      }
    }
    return true;
  }
  bool finish(CrSums& out) override {
    out = std::move(sums_);
    sums_ = CrSums();
    return true;
  }

 private:
  int N_;
  std::vector<double> epochs_;
  CrSums sums_;
};

}  // namespace

std::unique_ptr<CoalTreeWalker> make_host_walker(int N, const std::vector<double>& epochs) {
  return std::make_unique<HostWalker>(N, epochs);
}

}  // namespace colate_crt

// ------------------------------------------------------------------ C ABI: per-block sums from raw trees
namespace {

using namespace colate_crt;
using colate::fail;

int tree_accumulate(bool device, int N, int T, const int* parents, const double* branch_lengths, const double* weights,
                    const int* blocks, int num_blocks, const double* sample_ages, int E, const double* epochs, double* num,
                    double* denom) {
  const colate_cr::BlockAccumulate a{"coalrate tree", device, N, T, weights, blocks, num_blocks, E, epochs};
  if (const int rc = a.check_N()) return rc;
  if (T < 0 || num_blocks < 1 || E < 2 || E > 65535)
    return fail(COLATE_EINVAL, "coalrate tree: bad sizes (T %d, blocks %d, E %d)", T, num_blocks, E);
  if ((T && (!parents || !branch_lengths || !weights || !blocks)) || !epochs || !num || !denom)
    return fail(COLATE_EINVAL, "coalrate tree: NULL argument");
  if (const int rc = a.check_trees([](int) { return COLATE_OK; })) return rc;
  if (sample_ages)
    for (int i = 0; i < N; i++)
      if (!(sample_ages[i] >= 0.0)) return fail(COLATE_EINVAL, "coalrate tree: sample %d has age %g", i, sample_ages[i]);
  const std::vector<double> ep(epochs, epochs + E);
  const size_t nn = 2 * (size_t)N - 1;
  CrSums sums;
  const int rc = a.run<CrtChunk>(
      chunk_calls_for(N, E),
      [&](int chunk, std::string& err, int* code) { return device ? make_device_walker(-1, N, ep, chunk, err, code) : make_host_walker(N, ep); },
      [&](int t, CrtChunk& c, std::string& err) {
        const int k = c.append(N);
        c.w[k] = weights[t], c.block[k] = blocks[t];
        return prepare_times(N, sample_ages, ep, parents + t * nn, branch_lengths + t * nn, c.t.data() + k * nn, err);
      },
      sums);
  if (rc) return rc;
  std::fill(num, num + (size_t)num_blocks * E, 0.0);
  std::fill(denom, denom + (size_t)num_blocks * E, 0.0);
  const size_t n = (size_t)std::min(num_blocks, sums.blocks) * E;
  std::copy_n(sums.num.begin(), n, num);
  std::copy_n(sums.den.begin(), n, denom);
  return COLATE_OK;
}

}  // namespace

extern "C" int colate_coalrate_tree_accumulate(int N, int T, const int* parents, const double* branch_lengths, const double* weights,
                                               const int* blocks, int num_blocks, const double* sample_ages, int E,
                                               const double* epochs, double* num, double* denom) {
  colate_cr::launch_stats(colate_cr::kLaunchTree) = colate_cr::LaunchStats();
  return tree_accumulate(true, N, T, parents, branch_lengths, weights, blocks, num_blocks, sample_ages, E, epochs, num, denom);
}

extern "C" int colate_coalrate_tree_accumulate_host(int N, int T, const int* parents, const double* branch_lengths,
                                                    const double* weights, const int* blocks, int num_blocks,
                                                    const double* sample_ages, int E, const double* epochs, double* num,
                                                    double* denom) {
  return tree_accumulate(false, N, T, parents, branch_lengths, weights, blocks, num_blocks, sample_ages, E, epochs, num, denom);
}

extern "C" int colate_coalrate_tree_launch_shape(int* out) { return colate_cr::launch_stats(colate_cr::kLaunchTree).report(out); }
