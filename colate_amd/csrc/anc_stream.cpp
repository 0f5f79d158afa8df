// colate_amd/csrc/anc_stream.cpp -- anc_stream.h: the .anc reader and the worker pool of the tree-based estimators, and
// what the two CoalRate modes share around them.
#include "anc_stream.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <random>
#include <sstream>
#include <thread>

#include "colate_amd.h"

namespace colate_drv {

bool for_each_sliced(int nb, int nthreads, const SliceFn& fn, std::string& err) {
  std::vector<std::string> errs(nthreads);
  std::vector<std::thread> pool;
  const int per = (nb + nthreads - 1) / nthreads;
  for (int w = 0; w < nthreads; w++) {
    const int a = w * per, b = std::min(nb, a + per);
    if (a >= b) break;
    pool.emplace_back([&, a, b, w] {
      for (int k = a; k < b; k++)
        if (!fn(w, k, errs[w])) return;
    });
  }
  for (auto& th : pool) th.join();
  for (const std::string& e : errs)
    if (!e.empty()) {
      err = e;
      return false;
    }
  return true;
}

bool AncStream::open(const std::string& prefix) {
  prefix_ = prefix;
  return in_.open(prefix + ".anc") || in_.open(prefix + ".anc.gz");
}

bool AncStream::read_header(std::string& err) {
  std::string line;
  N = num_trees = 0;
  ages.clear();
  {  // mutations.cpp:555-581
    in_.getline(line);
    std::istringstream is(line);
    std::string tmp;
    is >> tmp >> N;
    if (N >= 2) {
      ages.resize(N);
      int i = 0;
      while (i < N && is >> ages[i]) i++;
      if (i != N) ages.clear();
    }
    in_.getline(line);
    std::istringstream is2(line);
    is2 >> tmp >> num_trees;
  }
  if (N < 2 || N > colate_cc::kMaxHaplotypes) {
    err = prefix_ + ".anc: " + std::to_string(N) + " haplotypes (colate_amd supports 2 .. " +
          std::to_string(colate_cc::kMaxHaplotypes) + ").";
    return false;
  }
  if (num_trees < 1) {
    err = prefix_ + ".anc has no trees.";
    return false;
  }
  first_ = 0;
  lines_.clear();
  return true;
}

bool AncStream::read_lines(int nb, std::string& err) {
  first_ += (int)lines_.size();
  lines_.resize(nb);
  for (int k = 0; k < nb; k++)
    if (!in_.getline(lines_[k])) {
      err = prefix_ + ".anc ends after " + std::to_string(first_ + k) + " of " + std::to_string(num_trees) + " trees.";
      return false;
    }
  return true;
}

bool AncStream::parse_lines(int nthreads, const std::function<bool(int k)>& wanted, const TreeFn& fn, std::string& err) const {
  struct Scratch {
    std::vector<int> par;
    std::vector<double> bl;
  };
  std::vector<Scratch> scratch(nthreads);
  const size_t nn = 2 * (size_t)N - 1;
  return for_each_sliced(
      (int)lines_.size(), nthreads,
      [&](int w, int k, std::string& e) {
        if (!wanted(k)) return true;
        Scratch& s = scratch[w];
        s.par.resize(nn);
        s.bl.resize(nn);
        if (!parse_tree_line(lines_[k], N, s.par.data(), s.bl.data())) {
          e = "cannot read tree " + std::to_string(first_ + k);
          return false;
        }
        std::string why;
        if (!fn(k, s.par.data(), s.bl.data(), why)) {
          e = "tree " + std::to_string(first_ + k) + ": " + why;
          return false;
        }
        return true;
      },
      err);
}

void plan_spans(const std::vector<MutRow>& rows, int num_trees, std::vector<TreeSpan>& plan) {
  const int L = (int)rows.size();
  plan.assign(num_trees, TreeSpan());
  int pit = 0, tim = rows[0].tree;
  for (int t = 0; t < num_trees; t++) {
    plan[t].it = std::min(pit, L - 1);  // (a tree after the last SNP: the reference dereferences the end of its list)
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
    plan[t].weight = (float)w;  // (the driver's float num_bases_tree_persists)
  }
}

// coal.cpp:267-325: the epochs in double from --bins (each field through stof)
static bool coalrate_epochs(const Options& opt, std::vector<double>& epochs, std::string& err) {
  const double log_10 = std::log(10);
  double years_per_gen = 28.0;
  if (opt.has("years_per_gen")) years_per_gen = std::stof(opt.get("years_per_gen"));
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
    try {
      v[k] = std::stof(tmp);
    } catch (...) {
      err = "Error: epochs format is wrong. Specify x,y,stepsize.";
      return false;
    }
  }
  const double epoch_lower = v[0], epoch_upper = v[1], epoch_step = v[2];
  if (!(epoch_step > 0)) {
    err = "Error: the step of --bins must be positive.";
    return false;
  }
  epochs.assign(1, 0.0);
  double epoch_boundary = epoch_lower;
  while (epoch_boundary < epoch_upper) {
    epochs.push_back(std::exp(log_10 * epoch_boundary) / years_per_gen);
    epoch_boundary += epoch_step;
  }
  epochs.push_back(std::exp(log_10 * epoch_upper) / years_per_gen);
  epochs.push_back(std::max(1e8, 10 * epochs[epochs.size() - 1]) / years_per_gen);
  for (size_t e = 1; e < epochs.size(); e++)
    if (!(epochs[e] > epochs[e - 1])) {
      err = "Error: the epochs of --bins do not increase.";
      return false;
    }
  return true;
}

bool CoalRateRun::read_settings(const Options& opt, const std::string& default_chr, const std::string& default_prefix) {
  std::string err;
  if (!coalrate_epochs(opt, epochs, err)) {
    std::cerr << err << std::endl;
    return false;
  }
  if (opt.has("num_bootstraps")) num_bootstrap = std::stoi(opt.get("num_bootstraps"));
  if (opt.has("seed")) (void)std::stoi(opt.get("seed"));  // (accepted; init_bootstrap seeds with 1 whatever it is)
  if (num_bootstrap < 1) {
    std::cerr << "Error: --num_bootstraps must be at least 1." << std::endl;
    return false;
  }
  if (opt.has("chr")) {
    GzText is;
    if (!is.open(opt.get("chr"))) {
      std::cerr << "Error while opening file " << opt.get("chr") << std::endl;
      return false;
    }
    std::string line;
    while (is.getline(line)) {
      chromosomes.push_back(line);
      prefixes.push_back(opt.get("input") + "_chr" + line);
    }
    if (chromosomes.empty()) {
      std::cerr << "Error: no chromosome in " << opt.get("chr") << std::endl;
      return false;
    }
  } else {
    chromosomes.push_back(default_chr);
    prefixes.push_back(default_prefix);
  }
  return true;
}

void CoalRateRun::choose_device(const Options& opt, bool by_default) {
  use_device_ = by_default;
  if (const char* e = std::getenv("COLATE_DEVICE_COALRATE")) {
    if (std::string(e) == "0") use_device_ = false;
    if (std::string(e) == "1") use_device_ = true;
  }
  if (use_device_ && colate_device_count() <= 0) use_device_ = false;  // no device: the host twin
  device_ = opt.has("device") ? std::stoi(opt.get("device")) : 0;
  nthreads = (int)std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
  timing_ = std::getenv("COLATE_TIMING") != nullptr;
  t_begin_ = StageTimes::now();
}

bool CoalRateRun::same_samples(const AncStream& anc, const std::string& prefix) {
  if (!n_) {
    n_ = anc.N;
    ages_ = anc.ages;
  } else if (anc.N != n_ || anc.ages != ages_) {
    std::cerr << "Error: " << prefix << ".anc has other haplotypes (or sample ages) than the first chromosome's." << std::endl;
    return false;
  }
  return true;
}

void CoalRateRun::begin_chromosome(int num_trees) {
  current_block_ = num_blocks;
  count_trees_ = 0;
  num_blocks += (int)(num_trees / ((double)kBlockSize) + 1);
  perc_ = -1;
  tree_count_ = 0;
  chr_trees_ = num_trees;
}

void CoalRateRun::progress() {
  if ((int)(((double)tree_count_) / chr_trees_ * 100.0) > perc_) {
    perc_ = (int)(((double)tree_count_) / chr_trees_ * 100.0);
    std::cerr << "[" << perc_ << "%]\r";
  }
  tree_count_++;
}

bool CoalRateRun::write_coal(const std::string& output, const std::string& first_line, const colate_cr::CrSums& sums, size_t cells,
                             int draw_max, const RowsFn& rows) const {
  std::ofstream os(output + ".coal");
  if (!os) {
    std::cerr << "Error: cannot write " << output << ".coal" << std::endl;
    return false;
  }
  os << first_line << "\n";
  for (double e : epochs) os << e << " ";
  os << "\n";
  std::mt19937 rng;
  rng.seed(1);
  std::uniform_int_distribution<int> d(0, draw_max);
  std::vector<int> times(num_blocks);
  std::vector<double> bnum(cells), bden(cells);
  for (int iter = 0; iter < num_bootstrap; iter++) {
    std::fill(times.begin(), times.end(), 0);
    for (int b = 0; b < num_blocks; b++) {
      const int x = d(rng);
      if (x < num_blocks) times[x]++;
    }
    std::fill(bnum.begin(), bnum.end(), 0.0);
    std::fill(bden.begin(), bden.end(), 0.0);
    // (a block without trees is skipped: the reference's tree mode adds times[b] * 0.0 for it, and adding +0.0 to a sum
    // that started at +0.0, which is never -0.0, changes no bit of it)
    for (int b = 0; b < num_blocks; b++)
      if (times[b] > 0 && b < sums.blocks)
        for (size_t i = 0; i < cells; i++) {
          bnum[i] += times[b] * sums.num[b * cells + i];
          bden[i] += times[b] * sums.den[b * cells + i];
        }
    rows(os, iter, bnum.data(), bden.data());
  }
  os.close();
  return true;
}

int CoalRateRun::done() const {
  if (timing_)
    std::fprintf(stderr, "coalrate timing: read+prepare %.3f s, walk %.3f s (%s %.3f s), total %.3f s\n", t_prepare_, t_walk_,
                 gpu_s_ > 0 ? "device kernels" : "host twin", gpu_s_, StageTimes::now() - t_begin_);
  print_usage_footer();
  return 0;
}

}  // namespace colate_drv
