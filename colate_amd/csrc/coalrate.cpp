// colate_amd/csrc/coalrate.cpp -- `CoalRate` (include/coal/CoalRate.cpp).  --mode tree: coal at include/coal/coal.cpp:21-204
// over coal_tree (coalrate_tree.h / coalrate_tree.cpp: the computation; here its driver, run_tree).  --mode local_ancestry
// (coal_localancestry at
// include/coal/coal.cpp:206-590, coal_LA at include/coal/coal_tree.cpp:300-654): coalescence rates for every pair of
// groups from Relate genealogies, the groups being population labels or local-ancestry labels that change along the genome.
//
//   * the preparation of a call (a tree dated as Tree::GetCoordinates dates it, its internal nodes by (epoch, label));
//   * the tables per group vector, the host twin of the device's pair counting (coalrate.h: the formulas);
//   * the C ABI over raw trees (colate_coalrate_accumulate[_host]);
//   * the drivers (colate_coalrate_main): options; run_local_ancestry with both poplabels formats, the per-tree segment
//     walk with its fractions and its .coal rows; run_tree with its call packing and its rows.  What the two share (the
//     .anc stream, settings, 5000-tree blocks, block bootstrap, the frame of the .coal) is anc_stream.h's.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <limits>
#include <map>
#include <memory>
#include <random>
#include <sstream>
#include <string>
#include <thread>
#include <vector>

#include "anc_stream.h"
#include "coalrate.h"
#include "coalrate_tree.h"
#include "colate_amd.h"
#include "colate_internal.h"

namespace colate_cr {

int CrChunk::append(int n) {
  N = n;
  leaf.resize(leaf.size() + n);
  node.resize(node.size() + (n - 1));
  w.push_back(0.0);
  gv.push_back(0);
  block.push_back(0);
  return T++;
}

int CrChunk::append_from(const CrChunk& src, int k) {
  const size_t n = src.N;
  const int x = append(src.N);
  std::copy_n(src.leaf.begin() + k * n, n, leaf.begin() + x * n);
  std::copy_n(src.node.begin() + k * (n - 1), n - 1, node.begin() + x * (n - 1));
  w[x] = src.w[k], gv[x] = src.gv[k], block[x] = src.block[k];
  return x;
}

namespace {

// the epoch of a node time: epochs[e] < t <= epochs[e+1] (coal_tree.cpp:473; t = 0 in epoch 0); E - 1 beyond the last boundary
int node_epoch(const std::vector<double>& epochs, double t) {
  return (int)(std::lower_bound(epochs.begin() + 1, epochs.end(), t) - (epochs.begin() + 1));
}
// the epoch of a sample age: the first e with epochs[e+1] > a (coal_tree.cpp:507); E - 1 beyond the last boundary
int age_epoch(const std::vector<double>& epochs, double a) {
  return (int)(std::upper_bound(epochs.begin() + 1, epochs.end(), a) - (epochs.begin() + 1));
}

}  // namespace

bool prepare_call(const CrRun& run, const int* parent, const double* bl, CrChunk& c, int k, std::string& err) {
  const int N = run.N, nn = 2 * N - 1, E = run.E();
  std::vector<int> lo(nn), hi(nn);
  int* leaf = c.leaf.data() + (size_t)k * N;
  if (!colate_cc::prepare_tree(N, parent, lo.data(), hi.data(), leaf, err)) return false;
  // node times, children before parents: coordinates[n] = max(coordinates[child] + branch_length) as a float (anc.cpp:280-308)
  const bool ancient = !run.ages.empty();
  std::vector<float> t(nn, 0.f);
  std::vector<double> best(nn, -std::numeric_limits<double>::infinity());
  std::vector<int> pending(nn, 2), ea(nn, 0), queue;
  queue.reserve(nn);
  for (int i = 0; i < N; i++) {
    if (ancient) {
      t[i] = (float)run.ages[i];
      ea[i] = age_epoch(run.epochs, run.ages[i]);
    }
    queue.push_back(i);
  }
  for (size_t h = 0; h < queue.size(); h++) {
    const int x = queue[h], p = parent[x];
    if (p < 0) continue;
    best[p] = std::max(best[p], (double)t[x] + bl[x]);
    ea[p] = std::max(ea[p], ea[x]);
    if (--pending[p] == 0) {
      t[p] = (float)best[p];
      queue.push_back(p);
    }
  }
  // epochs; the internal nodes by (epoch, label)
  std::vector<int> ev(nn, 0), first(E + 1, 0);
  for (int v = N; v < nn; v++) {
    const double tv = t[v];
    if (!(tv >= 0.0)) {
      err = "node " + std::to_string(v) + " has time " + std::to_string(tv);
      return false;
    }
    const int e = node_epoch(run.epochs, tv);
    if (e >= E - 1) {
      err = "node " + std::to_string(v) + " (time " + std::to_string(tv) + ") is older than the last epoch boundary " +
            std::to_string(run.epochs[E - 1]);
      return false;
    }
    if (e < ea[v]) {
      err = "node " + std::to_string(v) + " lies in an epoch below that of a sample age under it";
      return false;
    }
    ev[v] = e;
    first[e + 1]++;
  }
  for (int e = 0; e < E; e++) first[e + 1] += first[e];
  CrNode* node = c.node.data() + (size_t)k * (N - 1);
  std::vector<int> mid(nn, 0);
  for (int x = 0; x < nn - 1; x++) {
    const int p = parent[x];
    mid[p] = (lo[x] == lo[p]) ? hi[x] : lo[x];
  }
  for (int v = N; v < nn; v++) {
    CrNode& nd = node[first[ev[v]]++];
    nd.lo = (unsigned short)lo[v];
    nd.mid = (unsigned short)mid[v];
    nd.hi = (unsigned short)hi[v];
    nd.ev = (unsigned short)ev[v];
    nd.dt = (double)t[v] - run.epochs[ev[v]];
  }
  return true;
}

bool make_tables(const CrRun& run, CrTables& tab, std::string& err) {
  const int N = run.N, G = run.G, S = run.S, E = run.E(), GP = run.GP();
  tab.width.assign(E, 0.0);
  for (int e = 0; e + 1 < E; e++) tab.width[e] = run.epochs[e + 1] - run.epochs[e];
  // the leaves by (age, label) and the occupied age epochs
  std::vector<int> order(N), ea(N, 0);
  for (int i = 0; i < N; i++) order[i] = i;
  tab.oa_epoch.clear();
  if (run.ages.empty()) {
    tab.oa_epoch.push_back(0);
  } else {
    for (int i = 0; i < N; i++) {
      if (!(run.ages[i] >= 0.0)) {
        err = "sample " + std::to_string(i) + " has age " + std::to_string(run.ages[i]);
        return false;
      }
      ea[i] = age_epoch(run.epochs, run.ages[i]);
      if (ea[i] >= E - 1) {
        err = "sample " + std::to_string(i) + " is older than the last epoch boundary";
        return false;
      }
      tab.oa_epoch.push_back(ea[i]);
    }
    std::sort(tab.oa_epoch.begin(), tab.oa_epoch.end());
    tab.oa_epoch.erase(std::unique(tab.oa_epoch.begin(), tab.oa_epoch.end()), tab.oa_epoch.end());
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return run.ages[a] < run.ages[b]; });
  }
  tab.OA = (int)tab.oa_epoch.size();
  std::vector<int> slot(E, 0);
  for (int o = 0; o < tab.OA; o++) slot[tab.oa_epoch[o]] = o;
  tab.pairs.assign((size_t)S * tab.OA * GP, 0);
  tab.sub.assign((size_t)S * tab.OA * GP, 0.0);
  std::vector<long long> cnt(G);
  for (int s = 0; s < S; s++) {
    const int* grp = run.groups.data() + (size_t)s * N;
    for (int i = 0; i < N; i++)
      if (grp[i] < 0 || grp[i] >= G) {
        err = "group label " + std::to_string(grp[i]) + " outside 0.." + std::to_string(G - 1);
        return false;
      }
    std::fill(cnt.begin(), cnt.end(), 0);
    // a pair's age is its older sample's: leaf j, taken in order of age, pairs with every leaf before it
    for (int j : order) {
      const int gj = grp[j];
      const size_t at = ((size_t)s * tab.OA + slot[ea[j]]) * GP;
      const double over = run.ages.empty() ? 0.0 : run.ages[j] - run.epochs[ea[j]];
      for (int g = 0; g < G; g++) {
        if (!cnt[g]) continue;
        const int gp = cr_pair(std::max(g, gj), std::min(g, gj));
        tab.pairs[at + gp] += cnt[g];
        tab.sub[at + gp] += (double)cnt[g] * over;
      }
      cnt[gj]++;
    }
  }
  return true;
}

LaunchStats& launch_stats(LaunchMode mode) {
  static thread_local LaunchStats stats[2];
  return stats[mode];
}

size_t device_call_bytes(int N, int G, int E) {
  const size_t GP = (size_t)G * (G + 1) / 2;
  return sizeof(CrNode) * (N - 1) + sizeof(int) * N + (sizeof(int) + sizeof(double)) * E * GP + sizeof(unsigned short) * G * (N + 1) +
         32;
}

int chunk_calls_for(int N, int G, int E) {
  int calls = (int)std::max<size_t>(
      1, std::min<size_t>((4u << 20) / (unsigned)(2 * N - 1), ((size_t)256 << 20) / device_call_bytes(N, G, E)));
  if (const char* e = std::getenv("COLATE_COALRATE_CHUNK_TREES")) {
    const int k = std::atoi(e);
    if (k >= 1) calls = std::min(calls, k);
  }
  return calls;
}

namespace {

struct HostPre {
  const int* p;
  int n1;
  int operator()(int g, int q) const { return p[g * n1 + q]; }
};

class HostWalker final : public CoalRateWalker {
 public:
  HostWalker(const CrRun& run, const CrTables& tab) : run_(run), tab_(tab) {}
  bool submit(const CrChunk& c) override {
    const int N = run_.N, G = run_.G, E = run_.E(), GP = run_.GP(), n1 = N + 1, cells = E * GP;
    std::vector<int> pre((size_t)G * n1), cumB(cells);
    std::vector<double> R(cells);
    for (int k = 0; k < c.T; k++) {
      const int* leaf = c.leaf.data() + (size_t)k * N;
      const int* grp = run_.groups.data() + (size_t)c.gv[k] * N;
      std::fill(pre.begin(), pre.end(), 0);
      for (int q = 0; q < N; q++) {
        for (int g = 0; g < G; g++) pre[(size_t)g * n1 + q + 1] = pre[(size_t)g * n1 + q];
        pre[(size_t)grp[leaf[q]] * n1 + q + 1]++;
      }
      const HostPre rd{pre.data(), n1};
      for (int g1 = 0; g1 < G; g1++)
        for (int g2 = 0; g2 <= g1; g2++) {
          const int gp = cr_pair(g1, g2);
          cr_count_pair(N - 1, E, c.node.data() + (size_t)k * (N - 1), g1, g2, rd, cumB.data() + gp, R.data() + gp, (size_t)GP);
        }
      const int b = c.block[k];
      if (b >= sums_.blocks) {
        sums_.blocks = b + 1;
        sums_.num.resize((size_t)sums_.blocks * cells, 0.0);
        sums_.den.resize((size_t)sums_.blocks * cells, 0.0);
      }
      double* num = sums_.num.data() + (size_t)b * cells;
      double* den = sums_.den.data() + (size_t)b * cells;
      const size_t tab = (size_t)c.gv[k] * tab_.OA * GP;
      for (int e = 0; e < E; e++)
        for (int gp = 0; gp < GP; gp++) {
          const int cell = e * GP + gp;
          long long ca = 0;
          double sub = 0.0;
          for (int o = 0; o < tab_.OA; o++) {
            if (tab_.oa_epoch[o] <= e) ca += tab_.pairs[tab + (size_t)o * GP + gp];
            if (tab_.oa_epoch[o] == e) sub = tab_.sub[tab + (size_t)o * GP + gp];
          }
          cr_fold_cell(cumB[cell], e ? cumB[cell - GP] : 0, ca, R[cell], sub, tab_.width[e], c.w[k], num[cell], den[cell]);
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
  CrRun run_;
  CrTables tab_;
  CrSums sums_;
};

}  // namespace

std::unique_ptr<CoalRateWalker> make_host_walker(const CrRun& run, const CrTables& tab) {
  return std::make_unique<HostWalker>(run, tab);
}

}  // namespace colate_cr

// ------------------------------------------------------------------ C ABI: per-block sums from raw trees
namespace {

using namespace colate_cr;
using colate::fail;

int coalrate_accumulate(bool device, int N, int T, const int* parents, const double* branch_lengths, const double* weights,
                        const int* blocks, int num_blocks, const int* group_vector_ids, int S, const int* group_vectors, int G,
                        const double* sample_ages, int E, const double* epochs, double* num, double* denom) {
  const BlockAccumulate a{"coalrate", device, N, T, weights, blocks, num_blocks, E, epochs};
  if (const int rc = a.check_N()) return rc;
  if (T < 0 || num_blocks < 1 || S < 1 || G < 1 || E < 2 || E > 65535)
    return fail(COLATE_EINVAL, "coalrate: bad sizes (T %d, blocks %d, S %d, G %d, E %d)", T, num_blocks, S, G, E);
  if (G > 65535 || (long long)E * ((long long)G * (G + 1) / 2) > std::numeric_limits<int>::max())
    return fail(COLATE_ELIMIT, "coalrate: G = %d groups with E = %d epochs (G up to 65535, E * G * (G + 1) / 2 below 2^31)", G, E);
  if ((T && (!parents || !branch_lengths || !weights || !blocks || !group_vector_ids)) || !group_vectors || !epochs || !num || !denom)
    return fail(COLATE_EINVAL, "coalrate: NULL argument");
  const int rc_trees = a.check_trees([&](int t) {
    if (group_vector_ids[t] < 0 || group_vector_ids[t] >= S)
      return fail(COLATE_EINVAL, "coalrate: tree %d has group vector %d", t, group_vector_ids[t]);
    return (int)COLATE_OK;
  });
  if (rc_trees) return rc_trees;
  CrRun run;
  run.N = N, run.G = G, run.S = S;
  run.epochs.assign(epochs, epochs + E);
  if (sample_ages) run.ages.assign(sample_ages, sample_ages + N);
  run.groups.assign(group_vectors, group_vectors + (size_t)S * N);
  CrTables tab;
  std::string why;
  if (!make_tables(run, tab, why)) return fail(COLATE_EINVAL, "coalrate: %s", why.c_str());
  const int nn = 2 * N - 1;
  CrSums sums;
  const int rc = a.run<CrChunk>(
      chunk_calls_for(N, G, E),
      [&](int chunk, std::string& err, int* code) { return device ? make_device_walker(-1, run, tab, chunk, err, code) : make_host_walker(run, tab); },
      [&](int t, CrChunk& c, std::string& err) {
        if (weights[t] == 0.0) return true;  // (every addend a zero)
        const int k = c.append(N);
        c.w[k] = weights[t], c.gv[k] = group_vector_ids[t], c.block[k] = blocks[t];
        return prepare_call(run, parents + (size_t)t * nn, branch_lengths + (size_t)t * nn, c, k, err);
      },
      sums);
  if (rc) return rc;
  const int GP = run.GP();
  const size_t cells = (size_t)E * GP;
  std::fill(num, num + (size_t)num_blocks * G * G * E, 0.0);
  std::fill(denom, denom + (size_t)num_blocks * G * G * E, 0.0);
  for (int b = 0; b < num_blocks && b < sums.blocks; b++)
    for (int g1 = 0; g1 < G; g1++)
      for (int g2 = 0; g2 <= g1; g2++)
        for (int e = 0; e < E; e++) {
          const size_t to = (((size_t)b * G + g1) * G + g2) * E + e, from = b * cells + (size_t)e * GP + cr_pair(g1, g2);
          num[to] = sums.num[from];
          denom[to] = sums.den[from];
        }
  return COLATE_OK;
}

}  // namespace

extern "C" int colate_coalrate_accumulate(int N, int T, const int* parents, const double* branch_lengths, const double* weights,
                                          const int* blocks, int num_blocks, const int* group_vector_ids, int S,
                                          const int* group_vectors, int G, const double* sample_ages, int E, const double* epochs,
                                          double* num, double* denom) {
  launch_stats(kLaunchLocalAncestry) = LaunchStats();
  return coalrate_accumulate(true, N, T, parents, branch_lengths, weights, blocks, num_blocks, group_vector_ids, S, group_vectors,
                             G, sample_ages, E, epochs, num, denom);
}

extern "C" int colate_coalrate_accumulate_host(int N, int T, const int* parents, const double* branch_lengths,
                                               const double* weights, const int* blocks, int num_blocks,
                                               const int* group_vector_ids, int S, const int* group_vectors, int G,
                                               const double* sample_ages, int E, const double* epochs, double* num,
                                               double* denom) {
  return coalrate_accumulate(false, N, T, parents, branch_lengths, weights, blocks, num_blocks, group_vector_ids, S, group_vectors,
                             G, sample_ages, E, epochs, num, denom);
}

extern "C" int colate_coalrate_launch_shape(int* out) { return launch_stats(kLaunchLocalAncestry).report(out); }

// ------------------------------------------------------------------ the driver (CoalRate.cpp, coal.cpp:206-590)
namespace colate_drv {

namespace {

using namespace colate_cr;

const char* const kCoalRateOptions[] = {"mode", "anc", "mut", "chr", "bins", "years_per_gen", "seed", "num_bootstraps", "poplabels",
                                        "input", "output", "device"};

// CoalRate.cpp:11-23 (an unknown option is an error there too); ours: --device N
bool parse_coalrate_options(int argc, char** argv, Options& o, std::string& err) {
  for (int i = 1; i < argc; i++) {
    const std::string a = argv[i];
    std::string name, value;
    bool have_value = false;
    if (a.rfind("--", 0) == 0) {
      name = a.substr(2);
      const size_t eq = name.find('=');
      if (eq != std::string::npos) {
        value = name.substr(eq + 1);
        name = name.substr(0, eq);
        have_value = true;
      }
    } else if (a == "-i") {
      name = "input";
    } else if (a == "-o") {
      name = "output";
    } else {
      err = "Unexpected argument '" + a + "'";
      return false;
    }
    if (name == "help") {
      o.kv[name] = "true";
      continue;
    }
    if (std::find_if(std::begin(kCoalRateOptions), std::end(kCoalRateOptions), [&](const char* k) { return name == k; }) ==
        std::end(kCoalRateOptions)) {
      err = "Option '" + name + "' does not exist";
      return false;
    }
    if (!have_value) {
      if (i + 1 >= argc) {
        err = "Option '" + name + "' is missing an argument";
        return false;
      }
      value = argv[++i];
    }
    o.kv[name] = value;
  }
  return true;
}

void print_coalrate_help() {
  std::cout << "Usage:\n  CoalRate [OPTION...]\n\n"
            << "      --help                Print help.\n"
            << "      --mode arg            Choose which part of the algorithm to run (colate_amd: tree, local_ancestry).\n"
            << "      --chr arg             Optional: File specifying chromosomes to use.\n"
            << "      --bins arg            Epoch boundaries 10^(seq(x,y,stepsize)) [format: x,y,stepsize].\n"
            << "      --years_per_gen arg   Optional: Years per generation.\n"
            << "      --seed arg            Optional: Seed for random number generator (int)\n"
            << "      --num_bootstraps arg  Optional: Number of bootstraps.\n"
            << "      --poplabels arg       Population labels: the 4 column Relate poplabels format, or the local ancestry format\n"
            << "                            (all labels in the first row, then rows of chrom BP and one integer label per haplotype).\n"
            << "  -i, --input arg           Filename of input.\n"
            << "  -o, --output arg          Filename of output.\n"
            << "      --device arg          GPU ordinal (colate_amd).\n"
            << std::endl;
}

int count_tokens(const std::string& line) {
  std::istringstream is(line);
  std::string tok;
  int n = 0;
  while (is >> tok) n++;
  return n;
}

// The local-ancestry segments of a run: per segment its chromosome, first base and group vector.
struct Segments {
  std::vector<std::string> chrom, labels;
  std::vector<int> bp;
  std::vector<std::vector<int>> group;
};

// coal.cpp:403-461: the local ancestry format.  A header row of labels, then `chr bp label...` rows; the first row of a
// chromosome is at bp 0, and every row has one label per haplotype (the first row's count is checked against the .anc later).
bool read_local_ancestry(const std::string& path, Segments& seg, std::string& err) {
  GzText is;
  if (!is.open(path)) {
    err = "Error: Failed to open " + path;
    return false;
  }
  std::string line, tok;
  is.getline(line);
  {
    std::istringstream hs(line);
    while (hs >> tok) seg.labels.push_back(tok);
  }
  std::string current_chr;
  for (int row = 2; is.getline(line); row++) {
    if (line.empty()) continue;
    std::istringstream ls(line);
    std::string chr;
    int bp = 0;
    if (!(ls >> chr >> bp)) {
      err = "Error: line " + std::to_string(row) + " of " + path + " has no chromosome and BP";
      return false;
    }
    if ((seg.chrom.empty() || chr != current_chr) && bp != 0) {
      err = "Error: First entry for new chr has to start at BP = 0";
      return false;
    }
    current_chr = chr;
    std::vector<int> g;
    int val;
    while (ls >> val) g.push_back(val);
    if (!seg.group.empty() && g.size() != seg.group[0].size()) {
      err = "Error: line " + std::to_string(row) + " of " + path + " has " + std::to_string(g.size()) + " labels, the first row has " +
            std::to_string(seg.group[0].size());
      return false;
    }
    seg.chrom.push_back(chr);
    seg.bp.push_back(bp);
    seg.group.push_back(std::move(g));
  }
  if (seg.group.empty()) {
    err = "Error: " + path + " has no segments";
    return false;
  }
  return true;
}

// The banner of a mode, or why it does not start: the help, or the options it needs and has not got (-1: go on).
int coalrate_preamble(const Options& opt, std::initializer_list<const char*> needed, const char* needed_text, bool explain) {
  if (std::any_of(needed.begin(), needed.end(), [&](const char* k) { return !opt.has(k); })) {
    std::cout << "Not enough arguments supplied." << std::endl;
    std::cout << needed_text << std::endl;
    print_coalrate_help();
    if (explain) std::cout << "Calculate coalescence rates for sample." << std::endl;
    return 1;
  }
  if (opt.has("help")) {
    print_coalrate_help();
    std::cout << "Calculate coalescence rates for sample." << std::endl;
    return 0;
  }
  std::cerr << "---------------------------------------------------------" << std::endl;
  std::cerr << "Calculating coalescence rates for (ancient) sample.." << std::endl;
  return -1;
}

bool read_snps(const std::string& prefix, std::vector<MutRow>& rows) {
  read_mut_file(prefix + ".mut", rows);
  if (rows.empty()) std::cerr << "Error: " << prefix << ".mut has no SNPs." << std::endl;
  return !rows.empty();
}

// coal.cpp:206-590 over coal_LA (coal_tree.cpp:300-654): the coalescence rates of every pair of groups.
int run_local_ancestry(const Options& opt) {
  const int rc = coalrate_preamble(opt, {"input", "output", "poplabels", "bins"},
                                   "Needed: input, output, poplabels, bins. Optional: years_per_gen, chr, num_bootstraps", false);
  if (rc >= 0) return rc;
  CoalRateRun r;
  if (!r.read_settings(opt, "NA", opt.get("input"))) return 1;
  const std::vector<std::string>& chromosomes = r.chromosomes;
  std::string err;
  CrRun run;
  run.epochs = r.epochs;

  // the poplabels: four tokens in each of the first two lines mean the 4 column format (coal.cpp:364-381)
  Segments seg;
  {
    GzText is;
    if (!is.open(opt.get("poplabels"))) {
      std::cerr << "Error: Failed to open " << opt.get("poplabels") << std::endl;
      return 1;
    }
    std::string l1, l2;
    is.getline(l1);
    is.getline(l2);
    if (count_tokens(l1) == 4 && count_tokens(l2) == 4) {
      std::cerr << "Assuming 4 column poplabels file" << std::endl;
      Poplabels pl;
      if (!read_poplabels(opt.get("poplabels"), pl, err)) {
        std::cerr << err << std::endl;
        return 1;
      }
      seg.labels = pl.groups;
      for (size_t chr = 0; chr < chromosomes.size(); chr++) {  // two pseudo-segments per chromosome (coal.cpp:392-401)
        std::vector<MutRow> rows;
        if (!read_snps(r.prefixes[chr], rows)) return 1;
        seg.chrom.push_back(chromosomes[chr]);
        seg.bp.push_back(0);
        seg.chrom.push_back(chromosomes[chr]);
        seg.bp.push_back((int)(rows.back().pos + 1e6));
        seg.group.push_back(pl.group_of_haplotype);
        seg.group.push_back(pl.group_of_haplotype);
      }
    } else {
      std::cerr << "Assuming loc ancestry poplabels file" << std::endl;
      if (!read_local_ancestry(opt.get("poplabels"), seg, err)) {
        std::cerr << err << std::endl;
        return 1;
      }
    }
  }
  const int S = (int)seg.group.size();
  run.G = (int)seg.labels.size();
  run.S = S;
  if (run.G < 1) {
    std::cerr << "Error: " << opt.get("poplabels") << " names no group." << std::endl;
    return 1;
  }
  if (run.G > 65535 || (long long)run.E() * ((long long)run.G * (run.G + 1) / 2) > std::numeric_limits<int>::max()) {
    std::cerr << "Error: " << run.G << " groups with " << run.E() << " epochs are more than colate_amd supports." << std::endl;
    return 1;
  }
  r.choose_device(opt, true);

  std::unique_ptr<CoalRateWalker> walker;
  int chunk_calls = 1, local_index = 0;
  for (size_t chr = 0; chr < chromosomes.size(); chr++) {
    if (local_index == S) break;
    std::cerr << "CHR " << chromosomes[chr] << ":\n";
    const std::string& prefix = r.prefixes[chr];
    std::vector<MutRow> rows;
    if (!read_snps(prefix, rows)) return 1;
    AncStream anc;
    if (!anc.open(prefix)) {
      std::cerr << "Failed to open file " << prefix << ".anc(.gz)" << std::endl;
      return 1;
    }
    if (!anc.read_header(err)) {
      std::cerr << "Error: " << err << std::endl;
      return 1;
    }
    const int N = anc.N;
    if (!walker) {
      run.N = N;
      run.ages = anc.ages;
      run.groups.clear();
      for (const std::vector<int>& g : seg.group) {
        if ((int)g.size() != N) {
          std::cerr << "Error: " << opt.get("poplabels") << " has " << g.size() << " labels per row, the .anc has " << N
                    << " haplotypes." << std::endl;
          return 1;
        }
        run.groups.insert(run.groups.end(), g.begin(), g.end());
      }
      CrTables tab;
      if (!make_tables(run, tab, err)) {
        std::cerr << "Error: " << err << std::endl;
        return 1;
      }
      chunk_calls = chunk_calls_for(N, run.G, run.E());
      walker = r.make_walker([&](int device, std::string& why) { return make_device_walker(device, run, tab, chunk_calls, why); },
                             [&] { return make_host_walker(run, tab); });
    }
    if (!r.same_samples(anc, prefix)) return 1;

    if (chromosomes.size() > 1 || chromosomes[chr] != "NA") {
      while (seg.chrom[local_index] != chromosomes[chr]) {
        local_index++;
        if (local_index == S) {
          std::cerr << "Error: chromosome " << chromosomes[chr] << " not found in " << opt.get("poplabels") << std::endl;
          return 1;
        }
      }
    }
    if (seg.bp[local_index] != 0) {
      std::cerr << "Error: First entry for new chr has to start at BP = 0" << std::endl;
      return 1;
    }
    r.begin_chromosome(anc.num_trees);
    std::vector<TreeSpan> plan;
    plan_spans(rows, anc.num_trees, plan);
    const int L = (int)rows.size();
    const bool any_chr = chromosomes[chr] == "NA";
    auto same_chr = [&](int k) { return seg.chrom[k] == chromosomes[chr] || any_chr; };

    CrChunk base, out;  // the trees of a batch as prepared; the calls made of them
    bool stop = false;  // (the reference leaves a chromosome's loop when a cut tree reaches the last segment)
    for (int t0 = 0; t0 < anc.num_trees && !stop; t0 += chunk_calls) {
      const int nb = std::min(anc.num_trees, t0 + chunk_calls) - t0;
      const double ts = StageTimes::now();
      base.clear();
      for (int k = 0; k < nb; k++) base.append(N);
      // (a tree of weight 0: every call of it adds zeros, and it is never submitted)
      if (!anc.read_lines(nb, err) ||
          !anc.parse_lines(
              r.nthreads, [&](int k) { return plan[t0 + k].weight != 0.0f; },
              [&](int k, const int* par, const double* bl, std::string& e) { return prepare_call(run, par, bl, base, k, e); }, err)) {
        std::cerr << "Error: " << err << std::endl;
        return 1;
      }
      // the segment walk (coal.cpp:489-566) and coal_LA::populate
      out.clear();
      for (int k = 0; k < nb && !stop; k++) {
        const int t = t0 + k;
        const double w_tree = plan[t].weight;
        auto populate = [&](double w, int s, bool new_tree) {
          const int block = r.block();
          if (w != 0.0 && w_tree != 0.0) {
            const int x = out.append_from(base, k);
            out.w[x] = w, out.gv[x] = s, out.block[x] = block;
          }
          if (new_tree) r.count_tree();
        };
        r.progress();
        const int it = plan[t].it;
        int bp_start = rows[it].pos;
        if (it != 0) bp_start = (bp_start + rows[it - 1].pos) / 2.0;
        int j = it;
        while (j < L && rows[j].tree == rows[it].tree) j++;
        // past the last SNP the reference reads one element beyond its list; here bp_end is the last SNP's position
        int bp_end = (j < L) ? (int)((rows[j].pos + rows[j - 1].pos) / 2.0) : rows[L - 1].pos;
        if (bp_end == bp_start) bp_end++;
        if (local_index < S - 1) {
          while (local_index < S - 1 && bp_start >= seg.bp[local_index + 1] && same_chr(local_index + 1)) local_index++;
        }
        if (local_index < S - 1 && bp_end > seg.bp[local_index + 1] && same_chr(local_index + 1)) {
          // the tree extends beyond its segment
          double frac = w_tree * (seg.bp[local_index + 1] - bp_start) / ((double)bp_end - bp_start);
          populate(frac, local_index, true);
          local_index++;
          if (local_index + 1 == S) {
            stop = true;
            break;
          }
          while (bp_end > seg.bp[local_index + 1] && same_chr(local_index + 1)) {  // whole segments within the tree
            frac = w_tree * (seg.bp[local_index + 1] - seg.bp[local_index]) / ((double)bp_end - bp_start);
            populate(frac, local_index, false);
            local_index++;
            if (local_index + 1 >= S) {
              if (local_index == S) local_index--;
              break;
            }
          }
          frac = (bp_end - seg.bp[local_index]) / ((double)bp_end - bp_start);  // (coal.cpp:550: not times the tree's weight)
          populate(frac, local_index, false);
        } else {
          populate(w_tree, local_index, true);
        }
      }
      if (!r.submit(*walker, out, ts)) return 1;
    }
    local_index++;
    std::cerr << std::endl;
  }
  CrSums sums;
  if (!r.finish(walker, sums)) return 1;

  // coal_LA::init_bootstrap and Dump (coal_tree.cpp:529-654): draws in 0 .. num_blocks - 1
  const int G = run.G, E = run.E(), GP = run.GP();
  std::string labels;
  for (const std::string& g : seg.labels) labels += g + " ";
  const auto rows = [&](std::ostream& os, int, const double* num, const double* den) {
    for (int i = 0; i < G; i++)
      for (int j = 0; j < G; j++) {
        os << i << " " << j << " ";
        const int gp = cr_pair(std::max(i, j), std::min(i, j));
        for (int e = 0; e < E; e++) os << num[(size_t)e * GP + gp] / den[(size_t)e * GP + gp] << " ";
        os << "\n";
      }
  };
  if (!r.write_coal(opt.get("output"), labels, sums, (size_t)E * GP, r.num_blocks - 1, rows)) return 1;
  return r.done();
}

// coal.cpp:21-204 over coal_tree (coal_tree.cpp:1-295): the coalescence rate of the whole sample.
int run_tree(const Options& opt) {
  const int rc = coalrate_preamble(opt, {"input", "output", "bins"},
                                   "Needed: input, output, bins. Optional: years_per_gen, chr, num_bootstraps", true);
  if (rc >= 0) return rc;
  CoalRateRun r;
  if (!r.read_settings(opt, "1", opt.get("input") + "_chr1")) return 1;
  // The host twin is the default: at both measured shapes (profiles/coalrate/coalrate_tree_bench.json) opening the device
  // costs more than the host twin's whole walk, and the run is slower end to end.  COLATE_DEVICE_COALRATE=1 asks for the kernel.
  r.choose_device(opt, false);
  const std::vector<double>& epochs = r.epochs;
  const int E = (int)epochs.size();

  std::string err;
  std::unique_ptr<colate_crt::CoalTreeWalker> walker;
  int chunk_calls = 1;
  for (size_t chr = 0; chr < r.chromosomes.size(); chr++) {
    std::cerr << "CHR " << r.chromosomes[chr] << ":\n";
    const std::string& prefix = r.prefixes[chr];
    AncStream anc;
    if (!anc.open(prefix)) {
      std::cerr << "Error: --mode tree: failed to open " << prefix << ".anc(.gz)" << std::endl;
      return 1;
    }
    {
      GzText probe;
      if (!probe.open(prefix + ".mut") && !probe.open(prefix + ".mut.gz")) {
        std::cerr << "Error: --mode tree: failed to open " << prefix << ".mut(.gz)" << std::endl;
        return 1;
      }
    }
    std::vector<MutRow> rows;
    if (!read_snps(prefix, rows)) return 1;
    if (!anc.read_header(err)) {
      std::cerr << "Error: " << err << std::endl;
      return 1;
    }
    const int N = anc.N;
    for (double a : anc.ages)
      if (!(a >= 0.0)) {
        std::cerr << "Error: " << prefix << ".anc: sample age " << a << std::endl;
        return 1;
      }
    if (!walker) {
      chunk_calls = colate_crt::chunk_calls_for(N, E);
      walker = r.make_walker(
          [&](int device, std::string& why) { return colate_crt::make_device_walker(device, N, epochs, chunk_calls, why); },
          [&] { return colate_crt::make_host_walker(N, epochs); });
    }
    if (!r.same_samples(anc, prefix)) return 1;
    r.begin_chromosome(anc.num_trees);
    std::vector<TreeSpan> plan;
    plan_spans(rows, anc.num_trees, plan);
    const size_t nn = 2 * (size_t)N - 1;
    const double* ages = anc.ages.empty() ? nullptr : anc.ages.data();
    colate_crt::CrtChunk out;
    std::vector<int> call_of;
    for (int t0 = 0; t0 < anc.num_trees; t0 += chunk_calls) {
      const int nb = std::min(anc.num_trees, t0 + chunk_calls) - t0;
      const double ts = StageTimes::now();
      if (!anc.read_lines(nb, err)) {
        std::cerr << "Error: " << err << std::endl;
        return 1;
      }
      // coal_tree::populate: every tree counts; a tree of weight 0 adds nothing and is not submitted
      out.clear();
      call_of.assign(nb, -1);
      for (int k = 0; k < nb; k++) {
        r.progress();
        const int block = r.block();
        if (plan[t0 + k].weight != 0.0f) {
          const int x = out.append(N);
          out.w[x] = plan[t0 + k].weight, out.block[x] = block;
          call_of[k] = x;
        }
        r.count_tree();
      }
      if (!anc.parse_lines(
              r.nthreads, [&](int k) { return call_of[k] >= 0; },
              [&](int k, const int* par, const double* bl, std::string& e) {
                return colate_crt::prepare_times(N, ages, epochs, par, bl, out.t.data() + call_of[k] * nn, e);
              },
              err)) {
        std::cerr << "Error: " << err << std::endl;
        return 1;
      }
      if (!r.submit(*walker, out, ts)) return 1;
    }
    std::cerr << std::endl;
  }
  CrSums sums;
  if (!r.finish(walker, sums)) return 1;

  // coal_tree::init_bootstrap and Dump (coal_tree.cpp:180-295): draws in 0 .. num_blocks, the last of which selects no block
  std::string replicates;
  for (int i = 0; i < r.num_bootstrap; i++) replicates += std::to_string(i) + " ";
  const auto rows = [&](std::ostream& os, int iter, const double* num, const double* den) {
    os << "0 " << iter << " ";
    for (int e = 0; e < E; e++) os << num[e] / den[e] << " ";
    os << "\n";
  };
  if (!r.write_coal(opt.get("output"), replicates, sums, (size_t)E, r.num_blocks, rows)) return 1;
  return r.done();
}

}  // namespace

}  // namespace colate_drv

extern "C" int colate_coalrate_main(int argc, char** argv) {
  using namespace colate_drv;
  Options opt;
  std::string err;
  if (!parse_coalrate_options(argc, argv, opt, err)) {
    std::cerr << err << std::endl;
    return 1;
  }
  if (!opt.has("mode")) {
    std::cout << "Not enough arguments supplied." << std::endl;
    print_coalrate_help();
    return opt.has("help") ? 0 : 1;
  }
  const std::string& mode = opt.get("mode");
  if (mode == "local_ancestry") {
    try {
      return run_local_ancestry(opt);
    } catch (const std::exception& e) {
      std::cerr << "Error: " << e.what() << std::endl;
      return 1;
    }
  }
  if (mode == "tree") {
    try {
      return run_tree(opt);
    } catch (const std::exception& e) {
      std::cerr << "Error: " << e.what() << std::endl;
      return 1;
    }
  }
  std::cout << "####### error #######" << std::endl;
  std::cout << "Invalid or missing mode." << std::endl;
  std::cout << "Options for --mode are:" << std::endl;
  std::cout << "tree, local_ancestry." << std::endl;
  return 1;
}
