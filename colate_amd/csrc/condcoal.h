// colate_amd/csrc/condcoal.h -- `Colate --mode CondCoalRates` inside libcolate_amd.so: what the host side (condcoal.cpp:
// readers, tree preparation, host twin, bootstrap and writer) and the device side (condcoal_kernel.hip,
// condcoal_pairs_kernel.hip; their common plumbing is condcoal_device.hpp) share.
#pragma once
#include <cstddef>
#include <cstdint>
#include <memory>
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
  // a copy of tree k at the end; returns its index
  int append_copy(int k);
};

// Checks one tree (2N-1 nodes, leaves 0..N-1 without children, every internal node with two children, the one root at
// 2N-2, every node below it) and fills its DFS leaf ranges and order.  False with a message otherwise.
bool prepare_tree(int N, const int* parent, int* lo, int* hi, int* leaf, std::string& err);

// The per-block sums of a run's tables: [table][block][slots], a block without trees empty.
using CcTables = std::vector<std::vector<std::vector<double>>>;

// One way to walk: the trees of a run go in chunk by chunk, the per-block sums come out.  Every implementation sums in the
// same order (per lane or focal haplotype in walk order, per tree over the focal haplotypes ascending, per block over the
// trees in input order), so their tables agree bit for bit.
class CcWalker {
 public:
  virtual ~CcWalker() = default;
  virtual bool submit(const CcChunk& c) = 0;
  virtual bool finish(CcTables& acc) = 0;  // one entry per table
  const std::string& error() const { return err_; }
  int error_code() const { return code_; }
  double gpu_seconds() const { return gpu_s_; }  // kernel time by events (0 for the host twin)

 protected:
  bool fail(const std::string& what, int code) {
    err_ = what;
    code_ = code;
    return false;
  }
  double gpu_s_ = 0;

 private:
  std::string err_;
  int code_ = 0;
};

// The host twin: one table per run, each walked on the calling thread.
std::unique_ptr<CcWalker> make_host_walker(std::vector<CcRun> runs);

// The device side.  Chunks of at most max_trees trees go in asynchronously (the caller prepares the next one meanwhile).
// Null, and the reason in `why`, when there is no device or the run does not fit (device -1: the calling thread's).
//   * one table (condcoal_kernel.hip): each tree's accumulators come back and are added into their block in tree order at
//     finish(); the trees' blocks may come in any order.
//   * one table per (focal group, conditional group) pair (condcoal_pairs_kernel.hip; cond_group -1: the empty group): one
//     prefix pass per tree serves every pair, and the (pair, focal haplotype) lanes of several pairs share a workgroup.  Each
//     pair's sums are the single walker's, in the same order.  The per-block sums stay on the device while the block is open;
//     trees arrive in non-decreasing block order, and a block comes back when it closes.  base: N, G, group, ages, epochs,
//     efocal (its focal / is_cond are not read).
std::unique_ptr<CcWalker> make_device_walker(int device, const CcRun& run, int max_trees, std::string& why);
std::unique_ptr<CcWalker> make_pairs_device_walker(int device, const CcRun& base, const std::vector<int>& focal_group,
                                                   const std::vector<int>& cond_group, int max_trees, std::string& why);
// device bytes of results per tree of a chunk of the pairs walker (for chunk_trees_for)
size_t pairs_per_tree_bytes(int N, int G, int P, int slots);

}  // namespace colate_cc

// Readers that `CoalRate` (coalrate.cpp) shares with the CondCoalRates driver (condcoal.cpp).
namespace colate_drv {

// One line of a .anc file, "pos: " then 2N-1 times "parent:(branch_length num_events SNP_begin SNP_end) ".
bool parse_tree_line(const std::string& line, int N, int* parent, double* bl);

struct Poplabels {  // sample.cpp:8-110
  std::vector<std::string> groups;  // sorted
  std::vector<int> group_of_haplotype;
};
bool read_poplabels(const std::string& path, Poplabels& pl, std::string& err);

}  // namespace colate_drv
