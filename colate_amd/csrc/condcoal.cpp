// colate_amd/csrc/condcoal.cpp -- `Colate --mode CondCoalRates` (include/coal/coal.cpp:5001-5585): conditional pairwise
// coalescence rates from Relate genealogies (.anc / .mut).
//
//   * readers: the .anc's tree lines (anc.cpp:6-45; its opening, its header and the pool that parses a chunk of lines are
//     anc_stream.h's, shared with CoalRate), the .mut's pos / dist / tree_index (for_each_mut_row), the poplabels (sample.cpp:8-110),
//     the fasta mask (read_fasta_mask);
//   * per tree, what NextTree (mutations.cpp:616-670) and the driver's loop make of it: the weight
//     num_bases_tree_persists, the 30 Mb genome block, the mask filter (cutoff 0.9), and the extra pass of the last tree
//     with factor -1 (NextTree returns -1 without reading a line, and the loop body runs once more on the same tree);
//   * the walks (condcoal_walk.hpp): on the device (condcoal_kernel.hip) in chunks while the next chunk is parsed, or in
//     the host twin here (no device, or COLATE_DEVICE_CONDCOAL=0);
//   * the block bootstrap and the table, in the reference's float arithmetic.
#include <unistd.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <fstream>
#include <functional>
#include <iostream>
#include <memory>
#include <random>
#include <sstream>
#include <string>
#include <thread>
#include <vector>

#include "anc_stream.h"
#include "colate_amd.h"
#include "colate_internal.h"
#include "condcoal.h"
#include "condcoal_walk.hpp"

namespace colate_cc {

int CcChunk::append(int n) {
  const size_t nn = 2 * (size_t)n - 1;
  N = n;
  parent.resize(parent.size() + nn);
  lo.resize(lo.size() + nn);
  hi.resize(hi.size() + nn);
  bl.resize(bl.size() + nn);
  leaf.resize(leaf.size() + n);
  factor.push_back(0.f);
  block.push_back(0);
  return T++;
}

int CcChunk::append_copy(int k) {
  const size_t n = N, nn = 2 * n - 1;
  const int x = append(N);
  std::copy_n(parent.begin() + k * nn, nn, parent.begin() + x * nn);
  std::copy_n(lo.begin() + k * nn, nn, lo.begin() + x * nn);
  std::copy_n(hi.begin() + k * nn, nn, hi.begin() + x * nn);
  std::copy_n(bl.begin() + k * nn, nn, bl.begin() + x * nn);
  std::copy_n(leaf.begin() + k * n, n, leaf.begin() + x * n);
  factor[x] = factor[k];
  block[x] = block[k];
  return x;
}

bool prepare_tree(int N, const int* parent, int* lo, int* hi, int* leaf, std::string& err) {
  const int nn = 2 * N - 1;
  std::vector<int> c0(nn, -1), c1(nn, -1);
  for (int v = 0; v < nn; v++) {
    const int p = parent[v];
    if (p == -1) {
      if (v != nn - 1) {
        err = "the root of a tree is node " + std::to_string(v) + ", not 2N-2 = " + std::to_string(nn - 1);
        return false;
      }
      continue;
    }
    if (p < N || p >= nn || p == v) {
      err = "node " + std::to_string(v) + " has parent " + std::to_string(p);
      return false;
    }
    if (c0[p] < 0) c0[p] = v;
    else if (c1[p] < 0) c1[p] = v;
    else {
      err = "node " + std::to_string(p) + " has more than two children";
      return false;
    }
  }
  if (parent[nn - 1] != -1) {
    err = "node 2N-2 is not the root";
    return false;
  }
  for (int v = N; v < nn; v++)
    if (c1[v] < 0) {
      err = "internal node " + std::to_string(v) + " has fewer than two children";
      return false;
    }
  // one DFS from the root: leaf ranges [lo, hi) and the leaf order (every node reached once, or the tree is not connected)
  std::vector<int> stack;
  stack.reserve(2 * (size_t)nn);
  stack.push_back(nn - 1);
  int pos = 0, seen = 0;
  while (!stack.empty()) {
    const int x = stack.back();
    stack.pop_back();
    if (x < 0) {
      hi[~x] = pos;
      continue;
    }
    if (++seen > nn) break;
    lo[x] = pos;
    if (x < N) {
      leaf[pos++] = x;
      hi[x] = pos;
    } else {
      stack.push_back(~x);
      stack.push_back(c1[x]);
      stack.push_back(c0[x]);
    }
  }
  if (seen != nn || pos != N) {
    err = "the tree's nodes are not all below its root";
    return false;
  }
  return true;
}

namespace {

struct HostAcc {
  double* p;
  void add(int c, double v) { p[c] += v; }
};

CcShared shared_of(const CcRun& run) {
  CcShared sh;
  sh.N = run.N;
  sh.G = run.G;
  sh.E = run.E();
  sh.EF = run.EF();
  sh.group = run.group.data();
  sh.is_cond = run.is_cond.data();
  sh.cond_empty = run.cond_empty ? 1 : 0;
  sh.ages = run.ages.empty() ? nullptr : run.ages.data();
  sh.epochs = run.epochs.data();
  sh.efocal = run.efocal.data();
  return sh;
}

// The host twin: adds the chunk's trees into acc[block][slots] (acc grows to the largest block).
void host_accumulate(const CcRun& run, const CcChunk& c, std::vector<std::vector<double>>& acc) {
  const CcShared sh = shared_of(run);
  const int N = run.N, nn = 2 * N - 1, G = run.G, S = run.slots();
  std::vector<int> pre((size_t)(G + 1) * (N + 1));
  for (int t = 0; t < c.T; t++) {
    const int* leaf = c.leaf.data() + (size_t)t * N;
    for (int row = 0; row <= G; row++) {
      int r = 0;
      for (int q = 0; q < N; q++) {
        pre[(size_t)row * (N + 1) + q] = r;
        const int x = leaf[q];
        r += (row < G) ? (run.group[x] == row) : (int)run.is_cond[x];
      }
      pre[(size_t)row * (N + 1) + N] = r;
    }
    CcTree tr;
    tr.parent = c.parent.data() + (size_t)t * nn;
    tr.bl = c.bl.data() + (size_t)t * nn;
    tr.lo = c.lo.data() + (size_t)t * nn;
    tr.hi = c.hi.data() + (size_t)t * nn;
    tr.leaf = leaf;
    tr.prefix = pre.data();
    tr.factor = c.factor[t];
    const int b = c.block[t];
    if ((int)acc.size() <= b) acc.resize(b + 1);
    if (acc[b].empty()) acc[b].assign(S, 0.0);
    HostAcc a{acc[b].data()};
    for (int f : run.focal) cc_focal_walk(sh, tr, f, a);
  }
}

class HostWalker final : public CcWalker {
 public:
  explicit HostWalker(std::vector<CcRun> runs) : runs_(std::move(runs)), acc_(runs_.size()) {}
  bool submit(const CcChunk& c) override {
    for (size_t k = 0; k < runs_.size(); k++) host_accumulate(runs_[k], c, acc_[k]);
    return true;
  }
  bool finish(CcTables& acc) override {
    acc = std::move(acc_);
    acc_.assign(runs_.size(), {});
    return true;
  }

 private:
  std::vector<CcRun> runs_;
  CcTables acc_;
};

}  // namespace

std::unique_ptr<CcWalker> make_host_walker(std::vector<CcRun> runs) { return std::make_unique<HostWalker>(std::move(runs)); }

CcRun pair_run(const CcRun& base, int focal_group, int cond_group) {
  CcRun run = base;
  run.focal.clear();
  run.is_cond.assign(run.N, 0);
  for (int i = 0; i < run.N; i++) {
    if (run.group[i] == focal_group) run.focal.push_back(i);
    if (run.group[i] == cond_group) run.is_cond[i] = 1;
  }
  run.cond_empty = std::find(run.is_cond.begin(), run.is_cond.end(), 1) == run.is_cond.end();
  return run;
}

int chunk_trees_for(int N, size_t per_tree_bytes) {
  int trees = (int)std::max<size_t>(1, std::min<size_t>((4u << 20) / (unsigned)(2 * N - 1),
                                                       ((size_t)256 << 20) / std::max<size_t>(1, per_tree_bytes)));
  if (const char* e = std::getenv("COLATE_CONDCOAL_CHUNK_TREES")) {
    const int k = std::atoi(e);
    if (k >= 1) trees = std::min(trees, k);
  }
  return trees;
}

size_t pairs_per_tree_bytes(int N, int G, int P, int slots) {
  return sizeof(double) * (size_t)P * slots + sizeof(int) * (size_t)G * (N + 1);
}

}  // namespace colate_cc

// ------------------------------------------------------------------ C ABI: per-block accumulators from raw trees
namespace {

using namespace colate_cc;
using colate::fail;

struct RawTrees {  // the trees as the ABI takes them
  int N, T;
  const int* parents;
  const double* branch_lengths;
  const float* factors;
  const int* blocks;
  int num_blocks;
};

int check_haplotypes(int N) {
  if (N >= 2 && N <= kMaxHaplotypes) return COLATE_OK;
  return fail(N < 2 ? COLATE_EINVAL : COLATE_ELIMIT, "condcoal: N = %d haplotypes (supported: 2 .. %d)", N, kMaxHaplotypes);
}

// what every table of a call shares
int base_run(CcRun& base, int N, int G, const int* group_of_hap, const double* sample_ages, int E, const float* epochs, int EF,
             const float* epochs_focal) {
  base.N = N;
  base.G = G;
  base.group.assign(group_of_hap, group_of_hap + N);
  for (int g : base.group)
    if (g < 0 || g >= G) return fail(COLATE_EINVAL, "condcoal: group index %d outside 0..%d", g, G - 1);
  if (sample_ages) base.ages.assign(sample_ages, sample_ages + N);
  base.epochs.assign(epochs, epochs + E);
  base.efocal.assign(epochs_focal, epochs_focal + EF);
  return COLATE_OK;
}

// The trees through a walker, and its tables into num / denom [P][num_blocks][EF][E][G].  `ordered`: the blocks must not
// decrease (the pairs walkers sum a block while it is open; the single ones by index).  make(chunk_trees, why): the walker
// for chunks of that size, or null; per_tree_bytes: what a device walker keeps per tree of a chunk.
int accumulate_tables(const RawTrees& in, bool ordered, bool device, size_t per_tree_bytes, int P, int S,
                      const std::function<std::unique_ptr<CcWalker>(int, std::string&)>& make, double* num, double* denom) {
  const int N = in.N, T = in.T, nn = 2 * N - 1;
  for (int t = 0; t < T; t++) {
    if (in.blocks[t] < 0 || in.blocks[t] >= in.num_blocks) return fail(COLATE_EINVAL, "condcoal: tree %d in block %d", t, in.blocks[t]);
    if (ordered && t && in.blocks[t] < in.blocks[t - 1])
      return fail(COLATE_EINVAL, "condcoal: tree %d: blocks decrease (%d after %d)", t, in.blocks[t], in.blocks[t - 1]);
  }
  if (device && colate_device_count() <= 0) return fail(COLATE_ENODEVICE, "condcoal: no usable HIP device");
  const int chunk_trees = std::max(1, std::min(T, chunk_trees_for(N, device ? per_tree_bytes : 0)));
  std::string err;
  const std::unique_ptr<CcWalker> w = make(chunk_trees, err);
  if (!w) return fail(COLATE_EHIP, "condcoal: %s", err.c_str());
  CcChunk c;
  for (int t0 = 0; t0 < T; t0 += chunk_trees) {
    c.clear();
    const int t1 = std::min(T, t0 + chunk_trees);
    for (int t = t0; t < t1; t++) {
      const int k = c.append(N);
      std::memcpy(c.parent.data() + (size_t)k * nn, in.parents + (size_t)t * nn, sizeof(int) * nn);
      std::memcpy(c.bl.data() + (size_t)k * nn, in.branch_lengths + (size_t)t * nn, sizeof(double) * nn);
      c.factor[k] = in.factors[t];
      c.block[k] = in.blocks[t];
      if (!prepare_tree(N, c.parent.data() + (size_t)k * nn, c.lo.data() + (size_t)k * nn, c.hi.data() + (size_t)k * nn,
                        c.leaf.data() + (size_t)k * N, err))
        return fail(COLATE_EINVAL, "condcoal: tree %d: %s", t, err.c_str());
    }
    if (!w->submit(c)) return fail(w->error_code() ? w->error_code() : COLATE_EHIP, "%s", w->error().c_str());
  }
  CcTables acc;
  if (!w->finish(acc)) return fail(w->error_code() ? w->error_code() : COLATE_EHIP, "%s", w->error().c_str());
  const size_t NS = (size_t)S / 2;
  for (int p = 0; p < P; p++)
    for (int b = 0; b < in.num_blocks; b++) {
      const bool have = b < (int)acc[p].size() && !acc[p][b].empty();
      double* n = num + ((size_t)p * in.num_blocks + b) * NS;
      double* d = denom + ((size_t)p * in.num_blocks + b) * NS;
      for (size_t i = 0; i < NS; i++) {
        n[i] = have ? acc[p][b][i] : 0.0;
        d[i] = have ? acc[p][b][NS + i] : 0.0;
      }
    }
  return COLATE_OK;
}

int condcoal_accumulate(bool device, int N, int T, const int* parents, const double* branch_lengths, const float* factors,
                        const int* blocks, int num_blocks, int G, const int* group_of_hap, int F, const int* focal, int C,
                        const int* cond, const double* sample_ages, int E, const float* epochs, int EF,
                        const float* epochs_focal, double* num, double* denom) {
  if (int rc = check_haplotypes(N)) return rc;
  if (T < 0 || num_blocks < 1 || G < 1 || F < 1 || C < 0 || E < 1 || EF < 1)
    return fail(COLATE_EINVAL, "condcoal: bad sizes (T %d, blocks %d, G %d, F %d, C %d, E %d, EF %d)", T, num_blocks, G, F, C, E, EF);
  if ((T && (!parents || !branch_lengths || !factors || !blocks)) || !group_of_hap || !focal || (C && !cond) || !epochs ||
      !epochs_focal || !num || !denom)
    return fail(COLATE_EINVAL, "condcoal: NULL argument");
  CcRun run;
  if (int rc = base_run(run, N, G, group_of_hap, sample_ages, E, epochs, EF, epochs_focal)) return rc;
  run.is_cond.assign(N, 0);
  for (int i = 0; i < C; i++) {
    if (cond[i] < 0 || cond[i] >= N) return fail(COLATE_EINVAL, "condcoal: conditional haplotype %d", cond[i]);
    run.is_cond[cond[i]] = 1;
  }
  run.cond_empty = (C == 0);
  for (int i = 0; i < F; i++)
    if (focal[i] < 0 || focal[i] >= N) return fail(COLATE_EINVAL, "condcoal: focal haplotype %d", focal[i]);
  run.focal.assign(focal, focal + F);
  auto make = [&](int chunk_trees, std::string& why) {
    return device ? make_device_walker(-1, run, chunk_trees, why) : make_host_walker({run});  // (-1: the calling thread's device)
  };
  return accumulate_tables({N, T, parents, branch_lengths, factors, blocks, num_blocks}, false, device, 0, 1, run.slots(), make,
                           num, denom);
}

// The same for P (focal group, conditional group) pairs: out [P][num_blocks][EF][E][G].  The host twin runs each pair
// as its own CcRun (condcoal_accumulate's host path, bit for bit); the device walks all pairs in one pass.
int condcoal_accumulate_pairs(bool device, int N, int T, const int* parents, const double* branch_lengths, const float* factors,
                              const int* blocks, int num_blocks, int G, const int* group_of_hap, int P, const int* focal_group,
                              const int* cond_group, const double* sample_ages, int E, const float* epochs, int EF,
                              const float* epochs_focal, double* num, double* denom) {
  if (int rc = check_haplotypes(N)) return rc;
  if (T < 0 || num_blocks < 1 || G < 1 || P < 1 || E < 1 || EF < 1)
    return fail(COLATE_EINVAL, "condcoal: bad sizes (T %d, blocks %d, G %d, P %d, E %d, EF %d)", T, num_blocks, G, P, E, EF);
  if ((T && (!parents || !branch_lengths || !factors || !blocks)) || !group_of_hap || !focal_group || !cond_group || !epochs ||
      !epochs_focal || !num || !denom)
    return fail(COLATE_EINVAL, "condcoal: NULL argument");
  CcRun base;
  if (int rc = base_run(base, N, G, group_of_hap, sample_ages, E, epochs, EF, epochs_focal)) return rc;
  std::vector<int> fg(focal_group, focal_group + P), cg(cond_group, cond_group + P);
  for (int p = 0; p < P; p++) {
    if (fg[p] < 0 || fg[p] >= G) return fail(COLATE_EINVAL, "condcoal: pair %d: focal group %d outside 0..%d", p, fg[p], G - 1);
    if (cg[p] < -1 || cg[p] >= G)
      return fail(COLATE_EINVAL, "condcoal: pair %d: conditional group %d outside -1..%d", p, cg[p], G - 1);
    if (std::find(base.group.begin(), base.group.end(), fg[p]) == base.group.end())
      return fail(COLATE_EINVAL, "condcoal: pair %d: focal group %d has no haplotype", p, fg[p]);
  }
  auto make = [&](int chunk_trees, std::string& why) {
    if (device) return make_pairs_device_walker(-1, base, fg, cg, chunk_trees, why);  // (-1: the calling thread's device)
    std::vector<CcRun> runs;
    for (int p = 0; p < P; p++) runs.push_back(pair_run(base, fg[p], cg[p]));
    return make_host_walker(std::move(runs));
  };
  const int S = base.slots();
  return accumulate_tables({N, T, parents, branch_lengths, factors, blocks, num_blocks}, true, device,
                           pairs_per_tree_bytes(N, G, P, S), P, S, make, num, denom);
}

}  // namespace

extern "C" int colate_condcoal_accumulate_pairs(int N, int T, const int* parents, const double* branch_lengths,
                                                const float* factors, const int* blocks, int num_blocks, int G,
                                                const int* group_of_hap, int P, const int* focal_group, const int* cond_group,
                                                const double* sample_ages, int E, const float* epochs, int EF,
                                                const float* epochs_focal, double* num, double* denom) {
  return condcoal_accumulate_pairs(true, N, T, parents, branch_lengths, factors, blocks, num_blocks, G, group_of_hap, P,
                                   focal_group, cond_group, sample_ages, E, epochs, EF, epochs_focal, num, denom);
}

extern "C" int colate_condcoal_accumulate_pairs_host(int N, int T, const int* parents, const double* branch_lengths,
                                                     const float* factors, const int* blocks, int num_blocks, int G,
                                                     const int* group_of_hap, int P, const int* focal_group,
                                                     const int* cond_group, const double* sample_ages, int E,
                                                     const float* epochs, int EF, const float* epochs_focal, double* num,
                                                     double* denom) {
  return condcoal_accumulate_pairs(false, N, T, parents, branch_lengths, factors, blocks, num_blocks, G, group_of_hap, P,
                                   focal_group, cond_group, sample_ages, E, epochs, EF, epochs_focal, num, denom);
}

extern "C" int colate_condcoal_accumulate(int N, int T, const int* parents, const double* branch_lengths, const float* factors,
                                          const int* blocks, int num_blocks, int G, const int* group_of_hap, int F,
                                          const int* focal, int C, const int* cond, const double* sample_ages, int E,
                                          const float* epochs, int EF, const float* epochs_focal, double* num, double* denom) {
  return condcoal_accumulate(true, N, T, parents, branch_lengths, factors, blocks, num_blocks, G, group_of_hap, F, focal, C,
                             cond, sample_ages, E, epochs, EF, epochs_focal, num, denom);
}

extern "C" int colate_condcoal_accumulate_host(int N, int T, const int* parents, const double* branch_lengths,
                                               const float* factors, const int* blocks, int num_blocks, int G,
                                               const int* group_of_hap, int F, const int* focal, int C, const int* cond,
                                               const double* sample_ages, int E, const float* epochs, int EF,
                                               const float* epochs_focal, double* num, double* denom) {
  return condcoal_accumulate(false, N, T, parents, branch_lengths, factors, blocks, num_blocks, G, group_of_hap, F, focal, C,
                             cond, sample_ages, E, epochs, EF, epochs_focal, num, denom);
}

// ------------------------------------------------------------------ the driver (coal.cpp:5001-5585)
namespace colate_drv {

using namespace colate_cc;

// anc.cpp:6-45 (MarginalTree::Read + Tree::ReadTree): "pos: " then 2N-1 times "parent:(branch_length num_events SNP_begin SNP_end) "
bool parse_tree_line(const std::string& line, int N, int* parent, double* bl) {
  const char* s = line.c_str();
  const size_t L = line.size();
  size_t i = 0;
  while (i < L && s[i] != ':') i++;
  i += 2;
  for (int v = 0; v < 2 * N - 1; v++) {
    if (i >= L) return false;
    char* e = nullptr;
    const long p = std::strtol(s + i, &e, 10);  // sscanf %d
    if (e == s + i || e[0] != ':' || e[1] != '(') return false;
    char* e2 = nullptr;
    const double b = std::strtod(e + 2, &e2);   // sscanf %lf
    if (e2 == e + 2) return false;
    parent[v] = (int)p;
    bl[v] = b;
    while (i < L && s[i] != ')' && s[i] != '\n') i++;
    i += 2;
  }
  return true;
}

bool read_poplabels(const std::string& path, Poplabels& pl, std::string& err) {
  std::vector<std::vector<std::string>> rows;
  {
    GzText is;
    if (!is.open(path)) {
      err = "Error while opening file " + path + ".";
      return false;
    }
    std::string line;
    is.getline(line);  // header
    while (is.getline(line)) {
      std::vector<std::string> cols;
      size_t i = 0;
      while (i < line.size()) {
        size_t j = i;
        while (j < line.size() && line[j] != ' ' && line[j] != '\t') j++;
        cols.push_back(line.substr(i, j - i));
        i = j + 1;
      }
      if (line.empty()) continue;
      if (cols.size() < 2) {
        err = "poplabels line without a population column: " + line;
        return false;
      }
      rows.push_back(cols);
    }
  }
  bool diploid = true;
  for (const auto& c : rows) {
    const std::string ploidy = c.size() > 3 ? c[3] : "";
    if (ploidy != "NA") {
      if (ploidy == "1") diploid = false;
      else if (!diploid) {
        err = "Error: Detected both haploid and diploid samples.";
        return false;
      }
    }
    if (std::find(pl.groups.begin(), pl.groups.end(), c[1]) == pl.groups.end()) pl.groups.push_back(c[1]);
  }
  std::sort(pl.groups.begin(), pl.groups.end());
  for (const auto& c : rows) {
    const int g = (int)(std::find(pl.groups.begin(), pl.groups.end(), c[1]) - pl.groups.begin());
    pl.group_of_haplotype.push_back(g);
    if (diploid) pl.group_of_haplotype.push_back(g);
  }
  return true;
}

namespace {

// coal.cpp:5072-5146 (float epochs)
bool condcoal_epochs(const Options& opt, float years_per_gen, std::vector<float>& epochs, std::string& err) {
  const float log_10 = std::log(10);
  epochs.clear();
  if (opt.has("bins")) {
    const std::string& str = opt.get("bins");
    double v[3];
    size_t i = 0;
    for (int k = 0; k < 3; k++) {
      std::string tmp;
      while (i < str.size() && str[i] != ',') tmp += str[i++];
      i++;
      if (k < 2 && i >= str.size()) {
        err = "Error: epochs format is wrong. Specify x,y,stepsize.";
        return false;
      }
      v[k] = std::stof(tmp);
    }
    const double epoch_lower = v[0], epoch_upper = v[1], epoch_step = v[2];
    epochs.push_back(0.0);
    double epoch_boundary = epoch_lower;
    while (epoch_boundary < epoch_upper) {
      epochs.push_back(std::exp(log_10 * epoch_boundary) / years_per_gen);
      epoch_boundary += epoch_step;
    }
    epochs.push_back(std::exp(log_10 * epoch_upper) / years_per_gen);
    epochs.push_back(std::max(1e8, 10.0 * epochs[epochs.size() - 1]) / years_per_gen);
  } else {
    const int num_epochs = 31;
    epochs.resize(num_epochs);
    epochs[0] = 0.0;
    epochs[1] = 1e3 / years_per_gen;
    for (int e = 2; e < num_epochs - 1; e++)
      epochs[e] = std::exp(log_10 * (3.0 + 4.0 * (e - 1.0) / (num_epochs - 3.0))) / years_per_gen;
    epochs[num_epochs - 1] = 1e8 / years_per_gen;
  }
  return true;
}

struct TreePlan {  // one tree as the driver's loop sees it
  float factor = 0.f;
  int bin = 0;
  bool pass = true;
};

// NextTree (mutations.cpp:616-670) and the loop of coal.cpp:5292-5393 without walking: weight, block and mask verdict of every tree.
// A tree after the last SNP has no SNP to take its block from (the reference dereferences the end of its list there): the last
// SNP's is used.
bool plan_trees(const std::vector<MutRow>& rows, int num_trees, int chr_bin, const std::string* mask, std::vector<TreePlan>& plan,
                std::string& err) {
  const int L = (int)rows.size();
  const int bin_size = 30e6;
  plan.assign(num_trees, TreePlan());
  int pit = 0, tim = rows[0].tree;
  for (int t = 0; t < num_trees; t++) {
    const int it = pit;  // it_mut
    double w = 0.0;
    if (t == tim && pit < L) {
      w = (pit != 0) ? rows[pit - 1].dist / 2.0 : 0.0;
      while (rows[pit].tree == tim) {
        w += rows[pit].dist;
        pit++;
        if (pit == L) break;
      }
      if (pit != L) {
        w -= rows[pit - 1].dist / 2.0;
        tim = rows[pit].tree;
      }
    }
    TreePlan& p = plan[t];
    p.factor = (float)w;  // (NextTree's double into the driver's float num_bases_tree_persists, then factor)
    const int i = std::min(it, L - 1);
    p.bin = rows[i].pos / bin_size + chr_bin;
    if (mask) {  // coal.cpp:5401-5432: passing fraction over the tree's span between SNP midpoints
      const int tree_index = rows[i].tree;
      int pos_start = rows[i].pos;
      if (i != 0) pos_start = (pos_start + rows[i - 1].pos) / 2;
      int pos_end = pos_start + 1;
      int j = i;
      while (rows[j].tree == tree_index) {
        j++;
        if (j == L) break;
      }
      if (j != L) pos_end = rows[j].pos;
      if (j != 0) pos_end = (pos_end + rows[j - 1].pos) / 2;
      if (!(pos_end > pos_start)) {
        err = "mask: empty span for tree " + std::to_string(t);
        return false;
      }
      double num_passing = 0.0;
      for (int pos = pos_start; pos < pos_end; pos++)
        if (pos >= 0 && (size_t)pos < mask->size() && (*mask)[pos] == 'P') num_passing += 1.0;
      num_passing /= (pos_end - pos_start);
      p.pass = num_passing >= 0.9;  // (the reference reads an option `cutoff` that its parser does not declare: always 0.9)
    }
  }
  return true;
}

double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// One table to write: the single run's --groups / --output, or one line of the --pairs list.
struct CcJob {
  std::string g1, g2, output;
  int line = 0;  // line of the --pairs list (0: the single run)
  std::string where() const { return line ? " (line " + std::to_string(line) + " of the --pairs list)" : ""; }
};

// `FOCAL,COND OUTPUT` per line, blank lines skipped; the groups token splits as --groups does.
bool read_condcoal_pairs(const std::string& path, std::vector<CcJob>& jobs, std::string& err) {
  std::ifstream is(path);
  if (!is) {
    err = "cannot read the --pairs list " + path;
    return false;
  }
  std::string line;
  for (int k = 1; std::getline(is, line); k++) {
    std::istringstream ss(line);
    std::vector<std::string> tok;
    std::string w;
    while (ss >> w) tok.push_back(w);
    if (tok.empty()) continue;
    if (tok.size() != 2) {
      err = "line " + std::to_string(k) + " of the --pairs list: expected `FOCAL,CONDITIONAL OUTPUT`, got " +
            std::to_string(tok.size()) + " tokens";
      return false;
    }
    for (const CcJob& j : jobs)
      if (j.output == tok[1]) {
        err = "line " + std::to_string(k) + " of the --pairs list: output " + tok[1] + " is also line " + std::to_string(j.line) + "'s";
        return false;
      }
    CcJob j;
    const size_t comma = tok[0].find(',');
    j.g1 = tok[0].substr(0, comma);
    j.g2 = comma == std::string::npos ? "" : tok[0].substr(comma + 1);
    j.output = tok[1];
    j.line = k;
    jobs.push_back(j);
  }
  if (jobs.empty()) {
    err = "the --pairs list " + path + " has no pairs";
    return false;
  }
  return true;
}

// The run for a list of tables (one: the single run; several: --pairs): every input file is read once and every tree
// walked once for all tables.  Each table is the one its single run writes, byte for byte.
int condcoal_tables(const Options& opt, const std::vector<CcJob>& jobs, bool pairs_mode) {
  const double t_begin = now_s();
  std::cerr << "---------------------------------------------------------" << std::endl;
  std::cerr << "Calculating conditional coalescence rate for " << opt.get("input") << " ..." << std::endl;

  std::vector<std::string> chr_names;
  if (opt.has("chr")) {
    GzText is;
    if (!is.open(opt.get("chr"))) {
      std::cerr << "Error while opening file " << opt.get("chr") << std::endl;
      return 1;
    }
    std::string line;
    while (is.getline(line)) chr_names.push_back(line);
    if (chr_names.empty()) {
      std::cerr << "Error: no chromosome in " << opt.get("chr") << std::endl;
      return 1;
    }
  }
  const bool per_chr = !chr_names.empty();
  if (!per_chr) chr_names.push_back("NA");

  float years_per_gen = 28.0;
  if (opt.has("years_per_gen")) years_per_gen = std::stof(opt.get("years_per_gen"));
  std::string err;
  CcRun base;  // what every table shares (N, G, groups, ages, epochs)
  if (!condcoal_epochs(opt, years_per_gen, base.epochs, err)) {
    std::cerr << err << std::endl;
    return 1;
  }
  const float log_10 = std::log(10);
  float lineage_bin = 1e5;
  if (opt.has("lineage_bin")) lineage_bin = std::stof(opt.get("lineage_bin"));
  base.efocal = {0, std::exp(log_10 * lineage_bin)};  // coal.cpp:5148-5156 (float: the default's 10^1e5 is inf)
  for (float& e : base.efocal) e /= years_per_gen;

  // the rng serves the bootstrap only: every table starts from the same seed (without --seed: one drawn for the run)
  int seed = std::time(0) + getpid();
  if (opt.has("seed")) seed = std::stoi(opt.get("seed"));

  Poplabels pl;
  if (!read_poplabels(opt.get("poplabels"), pl, err)) {
    std::cerr << err << std::endl;
    return 1;
  }
  const size_t P = jobs.size();
  std::vector<int> fg(P), cg(P);  // group indices (-1: not in the poplabels)
  for (size_t k = 0; k < P; k++) {
    const CcJob& j = jobs[k];
    std::cerr << j.g1 << "|" << j.g2 << std::endl;
    const auto f = std::find(pl.groups.begin(), pl.groups.end(), j.g1), c = std::find(pl.groups.begin(), pl.groups.end(), j.g2);
    fg[k] = f == pl.groups.end() ? -1 : (int)(f - pl.groups.begin());
    cg[k] = c == pl.groups.end() ? -1 : (int)(c - pl.groups.begin());
    if (pairs_mode && fg[k] < 0) {
      std::cerr << "Error: groups not found" << j.where() << std::endl;
      return 1;
    }
  }

  // device or host twin
  bool use_device = true;
  if (const char* e = std::getenv("COLATE_DEVICE_CONDCOAL"))
    if (std::string(e) == "0") use_device = false;
  if (use_device && colate_device_count() <= 0) use_device = false;  // no device: the host twin
  const int device = opt.has("device") ? std::stoi(opt.get("device")) : 0;
  const int nthreads = (int)std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
  const bool timing = std::getenv("COLATE_TIMING") != nullptr;

  std::unique_ptr<CcWalker> walker;
  double t_parse = 0, t_walk = 0;
  int bin = 0, chr_bin = 0, N = 0, chunk_trees = 1;
  for (size_t chr = 0; chr < chr_names.size(); chr++) {
    std::cerr << "CHR: " << chr_names[chr] << std::endl;
    const std::string base_name = per_chr ? opt.get("input") + "_chr" + chr_names[chr] : opt.get("input");
    double t0 = now_s();
    std::vector<MutRow> rows;
    read_mut_file(base_name + ".mut", rows);
    if (rows.empty()) {
      std::cerr << "Error: " << base_name << ".mut has no SNPs." << std::endl;
      return 1;
    }
    AncStream anc;
    if (!anc.open(base_name)) {
      std::cerr << "Failed to open file " << base_name << ".anc(.gz)" << std::endl;
      return 1;
    }
    if (!anc.read_header(err)) {
      std::cerr << "Error: " << err << std::endl;
      return 1;
    }
    const int n_chr = anc.N, num_trees = anc.num_trees;
    const std::vector<double>& ages = anc.ages;
    std::string line;
    if (chr == 0) {
      N = n_chr;
      base.N = N;
      base.G = (int)pl.groups.size();
      base.ages = ages;
      if ((int)pl.group_of_haplotype.size() < N) {
        std::cerr << "Error: " << opt.get("poplabels") << " lists " << pl.group_of_haplotype.size() << " haplotypes, the .anc has "
                  << N << "." << std::endl;
        return 1;
      }
      base.group.assign(pl.group_of_haplotype.begin(), pl.group_of_haplotype.begin() + N);
      std::vector<CcRun> runs(P);
      for (size_t k = 0; k < P; k++) {
        runs[k] = pair_run(base, fg[k], cg[k]);
        if (runs[k].focal.empty()) {
          std::cerr << "Error: groups not found" << jobs[k].where() << std::endl;
          return 1;
        }
      }
      chunk_trees = chunk_trees_for(N, pairs_mode ? pairs_per_tree_bytes(N, base.G, (int)P, base.slots()) : 0);
      if (!use_device) {
        walker = make_host_walker(std::move(runs));
      } else {
        std::string why;
        walker = pairs_mode ? make_pairs_device_walker(device, base, fg, cg, chunk_trees, why)
                            : make_device_walker(device, runs[0], chunk_trees, why);
        if (!walker) {
          std::cerr << "Error: CondCoalRates on device " << device << ": " << why << std::endl;
          return 1;
        }
      }
    } else if (n_chr != N || ages != base.ages) {
      std::cerr << "Error: " << base_name << ".anc has other haplotypes (or sample ages) than the first chromosome's." << std::endl;
      return 1;
    }
    std::string mask_seq;
    if (opt.has("mask")) read_fasta_mask(per_chr ? opt.get("mask") + "_chr" + chr_names[chr] + ".fa" : opt.get("mask"), mask_seq);
    std::vector<TreePlan> plan;
    if (!plan_trees(rows, num_trees, chr_bin, opt.has("mask") ? &mask_seq : nullptr, plan, err)) {
      std::cerr << "Error: " << err << std::endl;
      return 1;
    }
    t_parse += now_s() - t0;

    // stream the trees that contribute: parse a chunk on the pool, hand it over, read on
    const int nn = 2 * N - 1;
    std::vector<std::string> lines;
    std::vector<int> which;  // tree index of each line
    CcChunk c;
    auto flush = [&](bool last_chunk) -> bool {
      const double tp = now_s();
      c.clear();
      for (size_t k = 0; k < lines.size(); k++) c.append(N);
      const bool parsed = for_each_sliced((int)lines.size(), nthreads, [&](int, int k, std::string& e) {
        int* par = c.parent.data() + (size_t)k * nn;
        if (!parse_tree_line(lines[k], N, par, c.bl.data() + (size_t)k * nn)) {
          e = "cannot read tree " + std::to_string(which[k]);
          return false;
        }
        std::string why;
        if (!prepare_tree(N, par, c.lo.data() + (size_t)k * nn, c.hi.data() + (size_t)k * nn, c.leaf.data() + (size_t)k * N, why)) {
          e = "tree " + std::to_string(which[k]) + ": " + why;
          return false;
        }
        return true;
      }, err);
      if (!parsed) return false;
      for (size_t k = 0; k < lines.size(); k++) {
        c.factor[k] = plan[which[k]].factor;
        c.block[k] = plan[which[k]].bin;
      }
      if (last_chunk && !lines.empty() && which.back() == num_trees - 1 && plan.back().pass) {
        // the extra pass of the last tree with factor -1 (coal.cpp:5292-5293, 5399-5400)
        const size_t k = lines.size() - 1;
        if (c.factor[k] == 0.0f) {
          c.factor[k] = -1.0f;  // (a weight-0 last tree: only the extra pass adds anything)
        } else {
          const int x = c.append_copy((int)k);  // (its block is the last tree's too)
          c.factor[x] = -1.0f;
        }
      }
      lines.clear();
      which.clear();
      t_parse += now_s() - tp;
      const double tw = now_s();
      if (!walker->submit(c)) {
        err = walker->error();
        return false;
      }
      t_walk += now_s() - tw;
      return true;
    };
    t0 = now_s();
    for (int t = 0; t < num_trees; t++) {
      if (!anc.getline(line)) {
        std::cerr << "Error: " << base_name << ".anc ends after " << t << " of " << num_trees << " trees." << std::endl;
        return 1;
      }
      const bool last = (t == num_trees - 1);
      if (!plan[t].pass || (plan[t].factor == 0.0f && !last)) continue;  // (weight 0: every addend is a zero)
      lines.push_back(std::move(line));
      line = std::string();
      which.push_back(t);
      if ((int)lines.size() >= chunk_trees - 1 && !last) {
        t_parse += now_s() - t0;
        if (!flush(false)) {
          std::cerr << "Error: " << err << std::endl;
          return 1;
        }
        t0 = now_s();
      }
    }
    t_parse += now_s() - t0;
    if (!flush(true)) {
      std::cerr << "Error: " << err << std::endl;
      return 1;
    }
    bin = plan.back().bin;  // (the -1 pass's block: the last tree's)
    chr_bin = bin + 1;
  }
  const double tw = now_s();
  CcTables acc;  // [table][block][slots]
  if (!walker->finish(acc)) {
    std::cerr << "Error: " << walker->error() << std::endl;
    return 1;
  }
  t_walk += now_s() - tw;
  const double gpu_s = walker->gpu_seconds();
  walker.reset();

  // bootstrap and tables (coal.cpp:5513-5568), float as there
  const double t_out = now_s();
  const int num_blocks = bin + 1;
  const int E = base.E(), EF = base.EF(), G = base.G, NS = EF * E * G;
  int num_bootstrap = 1;
  if (opt.has("num_bootstraps")) num_bootstrap = std::stoi(opt.get("num_bootstraps"));
  for (size_t k = 0; k < P; k++) {
    std::vector<float> bnum((size_t)num_blocks * NS, 0.f), bden((size_t)num_blocks * NS, 0.f);
    for (int b = 0; b < num_blocks && b < (int)acc[k].size(); b++)
      if (!acc[k][b].empty())
        for (int i = 0; i < NS; i++) {
          bnum[(size_t)b * NS + i] = (float)acc[k][b][i];
          bden[(size_t)b * NS + i] = (float)acc[k][b][NS + i];
        }
    std::mt19937 rng;
    rng.seed(seed);
    std::uniform_int_distribution<int> dist_blocks(0, num_blocks - 1);
    std::vector<int> blocks(num_blocks);
    std::ofstream os(jobs[k].output);
    if (!os) {
      std::cerr << "Error: cannot write " << jobs[k].output << std::endl;
      return 1;
    }
    os << "boot lineage_epoch epoch.start group rate" << std::endl;
    std::vector<float> res_num(NS), res_den(NS);
    for (int iter = 0; iter < num_bootstrap; iter++) {
      if (num_bootstrap == 1) {
        std::fill(blocks.begin(), blocks.end(), 1.0);
      } else {
        std::fill(blocks.begin(), blocks.end(), 0.0);
        for (int block = 0; block < num_blocks; block++) blocks[dist_blocks(rng)] += 1.0;
      }
      std::fill(res_num.begin(), res_num.end(), 0.f);
      std::fill(res_den.begin(), res_den.end(), 0.f);
      for (int block = 0; block < num_blocks; block++)
        for (int i = 0; i < NS; i++) {
          res_num[i] += blocks[block] * bnum[(size_t)block * NS + i];
          res_den[i] += blocks[block] * bden[(size_t)block * NS + i];
        }
      for (int ep1 = 0; ep1 < EF; ep1++)
        for (int ep2 = 0; ep2 < E; ep2++)
          for (int i = 0; i < G; i++) {
            const int q = (ep1 * E + ep2) * G + i;
            os << iter << " " << base.efocal[ep1] << " " << base.epochs[ep2] << " " << pl.groups[i] << " "
               << res_num[q] / res_den[q] << std::endl;
          }
    }
    os.close();
  }
  const double t_end = now_s();
  if (timing)
    std::fprintf(stderr, "condcoal timing: parse %.3f s, walk %.3f s (%s %.3f s), bootstrap+write %.3f s, total %.3f s\n", t_parse,
                 t_walk, gpu_s > 0 ? "device kernels" : "host twin", gpu_s, t_end - t_out, t_end - t_begin);
  print_usage_footer();
  return 0;
}

}  // namespace

int run_condcoal(const Options& opt) {
  if (opt.has("map")) {
    std::cerr << "Error: --map (the recombination-rate filter of CondCoalRates) is not supported by colate_amd." << std::endl;
    return 1;
  }
  std::vector<CcJob> jobs;
  if (opt.has("pairs")) {
    if (opt.has("groups") || opt.has("output")) {
      std::cerr << "Error: --pairs takes the groups and outputs from its list: no --groups or --output with it." << std::endl;
      return 1;
    }
    if (!opt.has("input") || !opt.has("poplabels")) {
      std::cerr << "Error: --mode CondCoalRates needs --input and --poplabels." << std::endl;
      return 1;
    }
    std::string err;
    if (!read_condcoal_pairs(opt.get("pairs"), jobs, err)) {
      std::cerr << "Error: " << err << std::endl;
      return 1;
    }
    return condcoal_tables(opt, jobs, true);
  }
  if (!opt.has("input") || !opt.has("output")) {
    std::cout << "Not enough arguments supplied." << std::endl;
    std::cout << "Needed: input, output. Optional: years_per_gen, dist, bins, mask, mask_cutof, mask, mask_cutofff." << std::endl;
    return 0;
  }
  if (!opt.has("poplabels") || !opt.has("groups")) {
    std::cerr << "Error: --mode CondCoalRates needs --poplabels and --groups." << std::endl;
    return 1;
  }
  CcJob j;
  const std::string& groups = opt.get("groups");
  const size_t comma = groups.find(',');
  j.g1 = groups.substr(0, comma);
  j.g2 = comma == std::string::npos ? "" : groups.substr(comma + 1);
  j.output = opt.get("output");
  jobs.push_back(j);
  return condcoal_tables(opt, jobs, false);
}

}  // namespace colate_drv
