// colate_amd/csrc/condcoal.h -- `Colate --mode CondCoalRates` inside libcolate_amd.so: what the host side (condcoal.cpp:
// readers, tree preparation, host twin, bootstrap and writer) and the device side (condcoal_kernel.hip) share.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

namespace colate_cc {

// Largest number of haplotypes: m * count stays below 2^28, so every (integer weight x float addend) is exact in double.
constexpr int kMaxHaplotypes = 16384;

// What every tree of a run shares (the arrays behind CcShared, condcoal_walk.hpp).
struct CcRun {
  int N = 0, G = 0;
  std::vector<int> group;               // [N]
  std::vector<unsigned char> is_cond;   // [N]
  bool cond_empty = false;
  std::vector<int> focal;               // the focal haplotypes, ascending
  std::vector<double> ages;             // [N] or empty (modern path)
  std::vector<float> epochs, efocal;
  int E() const { return (int)epochs.size(); }
  int EF() const { return (int)efocal.size(); }
  int slots() const { return 2 * EF() * E() * G; }
};

// One (focal group, conditional group) pair of a run as a CcRun of its own (the host twin's input): the focal haplotypes
// are the focal group's, ascending; the conditionals the conditional group's (cond_group -1: the empty group).
CcRun pair_run(const CcRun& base, int focal_group, int cond_group);

// Trees per chunk: the most that fit 4M node entries and `per_tree_bytes` of device results within 256 MiB, or
// COLATE_CONDCOAL_CHUNK_TREES where that is set and smaller (tests cross chunk and block boundaries on small inputs).
int chunk_trees_for(int N, size_t per_tree_bytes);

// A chunk of prepared trees, back to back (node arrays [T][2N-1], leaf orders [T][N]).
struct CcChunk {
  int N = 0, T = 0;
  std::vector<int> parent, lo, hi, leaf, block;
  std::vector<double> bl;
  std::vector<float> factor;
  void clear() {
    T = 0;
    parent.clear(), lo.clear(), hi.clear(), leaf.clear(), block.clear(), bl.clear(), factor.clear();
  }
  // room for one more tree; returns its index
  int append(int n);
};

// Checks one tree (2N-1 nodes, leaves 0..N-1 without children, every internal node with two children, the one root at
// 2N-2, every node below it) and fills its DFS leaf ranges and order.  False with a message otherwise.
bool prepare_tree(int N, const int* parent, int* lo, int* hi, int* leaf, std::string& err);

// The host twin: adds the chunk's trees into acc[block][slots] (acc grows to the largest block).
void host_accumulate(const CcRun& run, const CcChunk& c, std::vector<std::vector<double>>& acc);

// The device side (condcoal_kernel.hip).  Chunks go in asynchronously (the caller prepares the next one meanwhile);
// each tree's accumulators come back and are added into acc[block] in tree order at finish() (bit for bit reproducible).
class CcDevice {
 public:
  // null, and the reason in `why`, when there is no device or the run does not fit (device -1: the calling thread's)
  static CcDevice* create(int device, const CcRun& run, int max_trees, std::string& why);
  ~CcDevice();
  bool submit(const CcChunk& c);
  bool finish(std::vector<std::vector<double>>& acc);
  const std::string& error() const { return err_; }
  int error_code() const { return code_; }
  double gpu_seconds() const { return gpu_s_; }

 private:
  CcDevice() = default;
  bool fail(const char* what, int code);
  bool drain(int slot);
  struct Impl;
  Impl* p_ = nullptr;
  std::string err_;
  int code_ = 0;
  double gpu_s_ = 0;
};

// The walks of many (focal group, conditional group) pairs on the device (condcoal_pairs_kernel.hip): one prefix pass per
// tree serves every pair, and the (pair, focal haplotype) lanes of several pairs share a workgroup.  Each pair's sums are
// the single path's (CcDevice), in the same order: per lane in walk order, per (tree, pair) over the pair's focal
// haplotypes ascending, per (block, pair) over the trees in input order.  The per-block sums stay on the device while
// the block is open; trees arrive in non-decreasing block order, and a block comes back when it closes.
class CcPairsDevice {
 public:
  // base: N, G, group, ages, epochs, efocal (its focal / is_cond are not read); cond_group -1: the empty group.
  static CcPairsDevice* create(int device, const CcRun& base, const std::vector<int>& focal_group,
                               const std::vector<int>& cond_group, int max_trees, std::string& why);
  ~CcPairsDevice();
  bool submit(const CcChunk& c);
  // acc[block]: [P][slots] (empty for a block without trees)
  bool finish(std::vector<std::vector<double>>& acc);
  const std::string& error() const { return err_; }
  int error_code() const { return code_; }
  double gpu_seconds() const { return gpu_s_; }
  // device bytes of results per tree of a chunk (for chunk_trees_for)
  static size_t per_tree_bytes(int N, int G, int P, int slots);

 private:
  CcPairsDevice() = default;
  bool fail(const char* what, int code);
  bool drain(int slot);
  bool launch(const CcChunk& c, int t0, int t1);
  struct Impl;
  Impl* p_ = nullptr;
  std::string err_;
  int code_ = 0;
  double gpu_s_ = 0;
};

}  // namespace colate_cc
