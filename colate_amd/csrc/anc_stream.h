// colate_amd/csrc/anc_stream.h -- the stream of trees that the tree-based estimators read (anc_stream.cpp), once:
//   * AncStream: a Relate .anc(.gz) opened, its header read and checked, its tree lines read chunk by chunk, and
//     for_each_sliced, the pool of workers that parses a chunk: for `Colate --mode CondCoalRates` (condcoal.cpp) and both
//     modes of `CoalRate` (coalrate.cpp);
//   * CoalRateRun: what the two CoalRate modes share around that stream: the run's settings, the choice between device
//     and host twin, NextTree's weights, the 5000-tree block counter, the progress and timing lines, the block bootstrap
//     and the frame of the .coal file.
#pragma once
#include <chrono>
#include <functional>
#include <iostream>
#include <memory>
#include <string>
#include <vector>

#include "coalrate.h"
#include "mut_inputs.h"

namespace colate_drv {

// Runs fn(w, k, err) for k in [0, nb) on at most nthreads workers, worker w over the contiguous slice
// [w * per, (w + 1) * per), per = ceil(nb / nthreads).  A worker stops at its first false; the message of the
// lowest-numbered worker that stopped comes back.
using SliceFn = std::function<bool(int w, int k, std::string& err)>;
bool for_each_sliced(int nb, int nthreads, const SliceFn& fn, std::string& err);

class AncStream {
 public:
  int N = 0, num_trees = 0;
  std::vector<double> ages;  // [N], or empty (no sample ages in the header)

  bool open(const std::string& prefix);  // prefix.anc, then prefix.anc.gz
  // The two header lines: N in 2 .. kMaxHaplotypes, at least one tree.  False with a message.
  bool read_header(std::string& err);
  bool getline(std::string& line) { return in_.getline(line); }
  // The next nb tree lines.  False with a message when the file ends before them.
  bool read_lines(int nb, std::string& err);
  // Parses those of the lines just read that are wanted(k) and hands each tree to fn(k, parent, bl, err), on at most
  // nthreads workers.  False with the message of the first tree that does not parse or that fn refuses.
  using TreeFn = std::function<bool(int k, const int* parent, const double* bl, std::string& err)>;
  bool parse_lines(int nthreads, const std::function<bool(int k)>& wanted, const TreeFn& fn, std::string& err) const;

 private:
  GzText in_;
  std::string prefix_;
  std::vector<std::string> lines_;
  int first_ = 0;  // the tree of lines_[0]
};

// NextTree's weight of every tree (mutations.cpp:616-670) and the .mut row it leaves it_mut at
struct TreeSpan {
  float weight = 0.f;
  int it = 0;
};
void plan_spans(const std::vector<MutRow>& rows, int num_trees, std::vector<TreeSpan>& plan);

class CoalRateRun {
 public:
  std::vector<double> epochs;
  int num_bootstrap = 1;
  std::vector<std::string> chromosomes, prefixes;  // --chr's names and INPUT_chrNAME, or the mode's single default
  int nthreads = 1;
  int num_blocks = 0;  // of the chromosomes begun so far

  // --bins, --num_bootstraps, --seed and --chr.  False after saying what is wrong.
  bool read_settings(const Options& opt, const std::string& default_chr, const std::string& default_prefix);
  // The device where COLATE_DEVICE_COALRATE says so (or, by_default, does not say "0") and there is one; starts the clock.
  void choose_device(const Options& opt, bool by_default);
  // dev(device, why) where the device was chosen, host() where not or where dev returns null (which is said).
  template <class Dev, class Host>
  auto make_walker(Dev dev, Host host) -> decltype(host()) {
    decltype(host()) w;
    if (use_device_) {
      std::string why;
      w = dev(device_, why);
      if (!w) std::cerr << "CoalRate: the host twin runs instead of device " << device_ << ": " << why << std::endl;
    }
    if (!w) w = host();
    return w;
  }

  // Keeps the first chromosome's haplotypes and sample ages; false, after saying so, when a later one has others.
  bool same_samples(const AncStream& anc, const std::string& prefix);
  // coal_tree / coal_LA::update_ancmut: the chromosome's blocks follow those of the chromosomes before it
  void begin_chromosome(int num_trees);
  void progress();  // the "[n%]" line, once per tree
  // populate's block counter: the block of the next call, and a tree counted into it
  int block() {
    if (count_trees_ == kBlockSize) {
      current_block_++;
      count_trees_ = 0;
    }
    return current_block_;
  }
  void count_tree() { count_trees_++; }

  // Books the time since `since` as preparation and the submit as walk.  False after printing the walker's error.
  template <class Walker, class Chunk>
  bool submit(Walker& walker, const Chunk& chunk, double since) {
    double ts = StageTimes::now();
    t_prepare_ += ts - since;
    if (!walker.submit(chunk)) {
      std::cerr << "Error: " << walker.error() << std::endl;
      return false;
    }
    t_walk_ += StageTimes::now() - ts;
    return true;
  }
  // The sums of the run; the walker goes.
  template <class Walker>
  bool finish(std::unique_ptr<Walker>& walker, colate_cr::CrSums& sums) {
    const double ts = StageTimes::now();
    if (!walker || !walker->finish(sums)) {
      std::cerr << "Error: " << (walker ? walker->error() : std::string("no chromosome was read")) << std::endl;
      return false;
    }
    t_walk_ += StageTimes::now() - ts;
    gpu_s_ = walker->gpu_seconds();
    walker.reset();
    return true;
  }

  // init_bootstrap and Dump (coal_tree.cpp:180-295, 529-654): OUTPUT.coal with `first_line`, the epochs and, per
  // replicate, what rows(os, iter, num, den) writes from the cells' sums over the drawn blocks.  The seed is 1; a block is
  // drawn num_blocks times from 0 .. draw_max, and a draw of num_blocks (tree mode's draw_max) selects no block.
  using RowsFn = std::function<void(std::ostream& os, int iter, const double* num, const double* den)>;
  bool write_coal(const std::string& output, const std::string& first_line, const colate_cr::CrSums& sums, size_t cells,
                  int draw_max, const RowsFn& rows) const;
  // The timing line (COLATE_TIMING) and the usage footer; the exit status of a run that got here.
  int done() const;

 private:
  static constexpr int kBlockSize = 5000;
  bool use_device_ = false, timing_ = false;
  int device_ = 0;
  int n_ = 0;  // the first chromosome's haplotypes (0: none read yet)
  std::vector<double> ages_;
  int current_block_ = 0, count_trees_ = 0, perc_ = -1, tree_count_ = 0, chr_trees_ = 0;
  double t_begin_ = 0, t_prepare_ = 0, t_walk_ = 0, gpu_s_ = 0;
};

}  // namespace colate_drv
