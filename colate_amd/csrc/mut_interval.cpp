// colate_amd/csrc/mut_interval.cpp -- `Colate --mode mut_interval`: interval-dated observations per genome block, read from
// a text file, through the block bootstrap and the EM fit (colate_bootstrap_em_interval_batch: both on the device, the
// weighted block sums never visit the host) to OUT.coal.  The reference has no such mode: it wrote and tested coal_EM for
// age_begin < age_end (coal_EM.cpp:153-468) but never put a loop around it; the driver follows mut() (coal.cpp:3071-3863)
// where the two overlap: epochs from --bins or --coal at age 0, the block weights of coal.cpp:3350-3357 from the run's
// std::mt19937, the reference's iteration limits, the .coal writer.
//
// The rows come from a file (--rows: how a line becomes a mutation's (kind, age_begin, age_end) is the caller's business),
// or from the inputs of `--mode mut` (--mut, --target_tmp, --reference_tmp): every SNP the pair uses, snapped to the age
// grid, is one observation of each kind (interval_cells.h), formed on the device by colate_interval_cells.
// With --pairs LIST the second form runs for every line of the list in one pass (colate_interval_fit_groups); with
// --samples LIST for every target x reference pair of a sample list, the pairs walked on the device
// (colate_interval_fit_samples).
#include <algorithm>
#include <cerrno>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <map>
#include <random>
#include <sstream>
#include <string>
#include <tuple>
#include <vector>

#include "cli_lists.h"
#include "cli_modes.h"
#include "colate_amd.h"
#include "interval_walk.h"
#include "mut_interval.h"
#include "walk_inputs.h"

namespace colate_drv {

namespace {

// the whole token as a double (strtod's syntax); false where nothing or not all of it parses
bool parse_double(const std::string& tok, double& v) {
  if (tok.empty()) return false;
  char* end = nullptr;
  errno = 0;
  v = std::strtod(tok.c_str(), &end);
  return end == tok.c_str() + tok.size();  // (out of range: +-inf or 0, which the checks below see)
}

// digits only, at most 18 of them
bool parse_block(const std::string& tok, long long& v) {
  if (tok.empty() || tok.size() > 18) return false;
  v = 0;
  for (char c : tok) {
    if (c < '0' || c > '9') return false;
    v = v * 10 + (c - '0');
  }
  return true;
}

}  // namespace

bool read_interval_rows(const std::string& path, double epoch0, IntervalRows& out, std::string& err) {
  out = IntervalRows();
  GzText is;
  if (!is.open(path)) {
    err = "cannot open " + path;
    return false;
  }
  struct Cell {
    long long block;
    int row;
    double weight;
  };
  std::vector<Cell> cells;  // in file order
  std::map<std::tuple<int, double, double>, int> row_of;
  std::map<long long, int> block_of;
  std::string line;
  for (size_t line_no = 1; is.getline(line); line_no++) {
    auto fail = [&](const std::string& what) {
      err = path + ", line " + std::to_string(line_no) + ": " + what;
      return false;
    };
    std::vector<std::string> tok;
    for (size_t i = 0; i < line.size();) {
      while (i < line.size() && (line[i] == ' ' || (line[i] >= '\t' && line[i] <= '\r'))) i++;
      size_t j = i;
      while (j < line.size() && !(line[j] == ' ' || (line[j] >= '\t' && line[j] <= '\r'))) j++;
      if (j > i) tok.push_back(line.substr(i, j - i));
      i = j;
    }
    if (tok.empty() || tok[0][0] == '#') continue;
    if (tok.size() != 5) return fail("expected `block kind age_begin age_end weight`, found " + std::to_string(tok.size()) + " fields");
    Cell c;
    if (!parse_block(tok[0], c.block)) return fail("the block '" + tok[0] + "' is not a non-negative integer");
    const int kind = tok[1] == "shared" ? 0 : tok[1] == "notshared" ? 1 : -1;
    if (kind < 0) return fail("unknown kind '" + tok[1] + "' (known: shared, notshared)");
    double a0, a1;
    if (!parse_double(tok[2], a0)) return fail("age_begin '" + tok[2] + "' is not a number");
    if (!parse_double(tok[3], a1)) return fail("age_end '" + tok[3] + "' is not a number");
    if (!parse_double(tok[4], c.weight)) return fail("the weight '" + tok[4] + "' is not a number");
    // (what colate_em_interval_calls refuses, em_interval_host.cpp)
    if (!(a0 >= 0.0) || !(a1 >= 0.0)) return fail("negative age or not a number (" + tok[2] + ", " + tok[3] + ")");
    if (!(a0 <= a1)) return fail("age_begin " + tok[2] + " > age_end " + tok[3]);
    if (!(a1 <= 0x1.fffffffffffffp+1023)) return fail("infinite age");
    if (!(epoch0 <= a0)) return fail("age_begin " + tok[2] + " lies before the first epoch");
    if (!(c.weight >= 0.0) || !(c.weight <= 0x1.fffffffffffffp+1023)) return fail("the weight " + tok[4] + " must be finite and not negative");
    const auto key = std::make_tuple(kind, a0, a1);
    auto it = row_of.find(key);
    if (it == row_of.end()) {
      if (out.kinds.size() >= 0x7fffffffu) return fail("too many distinct rows");
      it = row_of.emplace(key, (int)out.kinds.size()).first;
      out.kinds.push_back(kind), out.age_begin.push_back(a0), out.age_end.push_back(a1);
    }
    c.row = it->second;
    block_of[c.block] = 0;
    cells.push_back(c);
  }
  if (cells.empty()) {
    err = path + ": no rows";
    return false;
  }
  if (block_of.size() > 0x7fffffffu) {
    err = path + ": too many blocks";
    return false;
  }
  for (auto& b : block_of) {  // ascending ids
    b.second = (int)out.block_ids.size();
    out.block_ids.push_back(b.first);
  }
  out.nb = (int)out.block_ids.size(), out.R = (int)out.kinds.size();
  out.tables.assign((size_t)out.nb * out.R, 0.0);
  for (const Cell& c : cells) out.tables[(size_t)block_of[c.block] * out.R + c.row] += c.weight;
  return true;
}

// The used SNPs of --mut / --target_tmp / --reference_tmp as rows and per-block tables (interval_cells.h): the engine's walk
// (mut_pairs.cpp) gives the records, colate_interval_cells -- or its host twin after a line on stderr -- the cells.
static bool rows_from_mut(const Options& opt, bool on_host, const std::string& host_why, IntervalRows& out) {
  std::vector<std::string> names, mut_files;
  PairSpec pair;
  pair.target = opt.get("target_tmp"), pair.reference = opt.get("reference_tmp");
  chromosome_files(opt, names, mut_files, &pair.target_masks, &pair.ref_masks);
  std::vector<colate_interval_rec> recs;
  std::vector<int> blocks;
  int nb = 0;
  if (!collect_interval_records(names, mut_files, pair, recs, blocks, nb)) {
    std::cerr << "Error: the SNPs of the pair could not be walked." << std::endl;
    return false;
  }
  if (nb < 1) {
    std::cerr << "Error: no genome block (no chromosome was read)." << std::endl;
    return false;
  }
  out = IntervalRows();
  const int cap = (int)std::min<size_t>(COLATE_INTERVAL_MAX_ROWS, 2 * recs.size());
  out.kinds.resize((size_t)cap), out.age_begin.resize((size_t)cap), out.age_end.resize((size_t)cap), out.tables.resize((size_t)nb * cap);
  long long dropped = 0;
  if (on_host) std::cerr << "interval cells on the host (" << host_why << ")" << std::endl;
  const int R = (on_host ? colate_interval_cells_host : colate_interval_cells)(
      (long long)recs.size(), recs.data(), blocks.data(), nb, cap, out.kinds.data(), out.age_begin.data(), out.age_end.data(),
      out.tables.data(), &dropped);
  if (R < 0) return api_error(R), false;
  out.nb = nb, out.R = R;
  out.kinds.resize((size_t)R), out.age_begin.resize((size_t)R), out.age_end.resize((size_t)R), out.tables.resize((size_t)nb * R);
  for (int k = 0; k < nb; k++) out.block_ids.push_back(k);
  std::cerr << "Number of blocks: " << nb << std::endl;
  std::cerr << "Number of rows: " << R << std::endl;
  std::cerr << "SNPs beyond the age grid: " << dropped << std::endl;
  if (R == 0) {
    std::cerr << "Error: the pair uses no SNP within the age grid." << std::endl;
    return false;
  }
  return true;
}

// --write_rows: the rows in the --rows format, row by row and within a row the blocks ascending, one line per cell with a
// positive weight, 17 significant digits.  A block without any positive cell gets a line of weight 0 on the first row, so
// that reading the file back gives the same blocks, rows (in this order: first appearance) and tables.
static bool write_interval_rows(const std::string& path, const IntervalRows& rows) {
  FILE* f = std::fopen(path.c_str(), "w");
  if (!f) return false;
  std::fprintf(f, "# block kind age_begin age_end weight\n");
  std::vector<char> seen((size_t)rows.nb, 0);
  for (int k = 0; k < rows.nb; k++)
    for (int r = 0; r < rows.R && !seen[k]; r++) seen[k] = rows.tables[(size_t)k * rows.R + r] > 0.0;
  for (int r = 0; r < rows.R; r++)
    for (int k = 0; k < rows.nb; k++) {
      const double w = rows.tables[(size_t)k * rows.R + r];
      if (w > 0.0 || (r == 0 && !seen[k]))
        std::fprintf(f, "%lld %s %.17g %.17g %.17g\n", rows.block_ids[k], rows.kinds[r] == 0 ? "shared" : "notshared", rows.age_begin[r],
                     rows.age_end[r], w);
    }
  return std::fclose(f) == 0;
}

// What the runs of `--mode mut_interval` share (one pair, --pairs, --samples) besides the run's options: the choice between device
// and host twin, epochs and starting rates, and what is said and written per pair.
struct FitRun : RunOptions {
  using RunOptions::RunOptions;
  std::string host_why;  // not empty: the host twins run
  int status = 0;
};
// device or host twin (false after an error message)
static bool fit_run_device(const Options& opt, FitRun& run) {
  return choose_path("COLATE_DEVICE_INTERVAL", true, run.host_why) != Path::device || bind_device(opt);
}
// Epochs and starting rates at age 0, as for `mut` with a modern sample (coal.cpp:3501-3646): those of the .coal file where one
// is given, else --bins with the default starting rate.  False after `lead` and the library's message on stderr.
static bool fit_run_epochs(const Options& opt, const FitRun& run, const std::string* coal, const std::string& lead, std::vector<double>& epochs,
                           std::vector<double>& init, int& ep_null) {
  const bool ok = epochs_for(opt, coal, 0.0, run.years_per_gen, epochs, init, ep_null) > 0;
  if (!ok) std::cerr << lead << colate_last_error() << std::endl;
  return ok;
}
// the lines of pair p after its fit, and its .coal (rates: [B][E] of the pair)
static void report_pair(FitRun& run, size_t p, const PairSpec& ps, int R, long long dropped, int E, const double* epochs, int ep_null,
                        const double* rates, const int* iters, const int* flags) {
  const std::string lead = "Pair " + std::to_string(p + 1) + " ";
  std::cerr << lead << "Number of rows: " << R << std::endl;
  std::cerr << lead << "SNPs beyond the age grid: " << dropped << std::endl;
  if (R == 0) {
    std::cerr << "Error: pair " << p + 1 << " (" << ps.target << " x " << ps.reference << ") uses no SNP within the age grid; " << ps.output
              << ".coal is not written." << std::endl;
    run.status = 1;
    return;
  }
  report_bootstraps((int)p + 1, run.B, E, iters, flags, false);
  if (!write_coal(ps.output, run.B, E, epochs, rates, false, ep_null)) run.status = 1;
}

// The pairs of a list (`--pairs`, or the expanded list of `--samples` where its pairs cannot be walked over indices): every
// input file is read once and the pairs are walked on the pool (collect_interval_records_pairs; loaded: inputs read before);
// the pairs with the same number of epochs, in order of first appearance, go through one colate_interval_fit_groups call --
// cells, rows, block bootstrap and fit of all of them on the device, or the host twin after a line on stderr.  Every pair
// draws its block weights from a generator of its own on the run's seed, as its single run does, so OUTPUT.coal is that
// run's, byte for byte.
static int fit_pair_list(const Options& opt, FitRun& run, const std::vector<std::string>& names, const std::vector<std::string>& mut_files,
                         const std::vector<PairSpec>& pairs, const WalkInputs* loaded) {
  const size_t P = pairs.size();
  const int B = run.B;

  // ---- epochs and starting rates per pair: the line's coal=, else --bins, else --coal
  std::vector<std::vector<double>> epochs(P), init(P);
  std::vector<int> ep_null(P, 0);
  for (size_t p = 0; p < P; p++) {
    const std::string* coal = !pairs[p].coal.empty() ? &pairs[p].coal : nullptr;
    if (!coal && !opt.has("bins") && opt.has("coal") && !opt.get("coal").empty()) coal = &opt.get("coal");
    if (!fit_run_epochs(opt, run, coal, "Error: pair " + std::to_string(p + 1) + ": ", epochs[p], init[p], ep_null[p])) return 1;
  }

  // ---- the records of all pairs
  const double t_start = StageTimes::now();
  std::vector<PairRecords> recs;
  if (!(loaded ? collect_interval_records_loaded(*loaded, names, pairs, recs) : collect_interval_records_pairs(names, mut_files, pairs, recs)))
    return 1;
  const double t_fit = StageTimes::now();
  double kernel_s = 0.0;
  long long total_recs = 0;
  for (const PairRecords& pr : recs) total_recs += (long long)pr.recs.size();
  std::vector<char> usable(P, 1);
  for (size_t p = 0; p < P; p++) {
    say_blocks(p, P, pairs[p], recs[p].nb);
    if (!recs[p].walked || recs[p].nb < 1) {
      std::cerr << "Error: pair " << p + 1 << " (" << pairs[p].target << " x " << pairs[p].reference << "): "
                << (recs[p].walked ? "no genome block (no chromosome was read)." : "the SNPs of the pair could not be walked.") << std::endl;
      usable[p] = 0, run.status = 1;
    }
  }

  // ---- classes of pairs with the same number of epochs, in order of first appearance: one grouped call each
  const std::vector<std::vector<size_t>> classes = classes_by_epoch_count(epochs, &usable);
  std::cerr << "Maximising likelihood using EM.. " << std::endl;
  if (!run.host_why.empty()) std::cerr << "interval cells and fits on the host (" << run.host_why << ")" << std::endl;
  for (const std::vector<size_t>& cls : classes) {
    const int G = (int)cls.size(), E = (int)epochs[cls[0]].size();
    std::vector<long long> rec_off(1, 0);
    std::vector<int> nb;
    std::vector<double> weights, g_ep, g_init;
    for (size_t p : cls) {
      rec_off.push_back(rec_off.back() + (long long)recs[p].recs.size());
      nb.push_back(recs[p].nb);
      std::mt19937 rng(run.seed);  // (coal.cpp:3350-3357: every pair from the run's seed, as its single run)
      const size_t at = weights.size();
      weights.resize(at + (size_t)B * recs[p].nb);
      if (int rc = colate_bootstrap_weights(&rng, B, recs[p].nb, weights.data() + at)) return api_error(rc);
      g_ep.insert(g_ep.end(), epochs[p].begin(), epochs[p].end());
      g_init.insert(g_init.end(), init[p].begin(), init[p].end());
    }
    std::vector<colate_interval_rec> all_recs((size_t)rec_off.back());
    std::vector<int> all_blocks((size_t)rec_off.back());
    for (int g = 0; g < G; g++) {
      PairRecords& pr = recs[cls[(size_t)g]];
      std::copy(pr.recs.begin(), pr.recs.end(), all_recs.begin() + rec_off[(size_t)g]);
      std::copy(pr.blocks.begin(), pr.blocks.end(), all_blocks.begin() + rec_off[(size_t)g]);
      pr = PairRecords();  // (the pair's own copy is no longer needed)
    }
    const size_t GB = (size_t)G * B;
    std::vector<int> R(G), iters(GB), flags(GB);
    std::vector<long long> dropped(G);
    std::vector<double> rates(GB * E), ll(GB);
    const int rc = run.host_why.empty()
                       ? colate_interval_fit_groups(G, B, E, rec_off.data(), all_recs.data(), all_blocks.data(), nb.data(), weights.data(),
                                                    g_ep.data(), g_init.data(), run.max_iter, run.min_iter, COLATE_DEFAULT_REL_TOL,
                                                    COLATE_DEFAULT_RATE_FLOOR, R.data(), dropped.data(), rates.data(), iters.data(),
                                                    ll.data(), flags.data())
                       : colate_interval_fit_groups_host(G, B, E, rec_off.data(), all_recs.data(), all_blocks.data(), nb.data(),
                                                         weights.data(), g_ep.data(), g_init.data(), run.max_iter, run.min_iter,
                                                         COLATE_DEFAULT_REL_TOL, COLATE_DEFAULT_RATE_FLOOR, R.data(), dropped.data(),
                                                         rates.data(), iters.data(), ll.data(), flags.data(), 1);
    if (rc) return api_error(rc);
    if (run.host_why.empty()) kernel_s += colate_interval_fit_groups_kernel_seconds();
    for (int g = 0; g < G; g++) {
      const size_t p = cls[(size_t)g];
      report_pair(run, p, pairs[p], R[g], dropped[g], E, epochs[p].data(), ep_null[p], rates.data() + (size_t)g * B * E,
                  iters.data() + (size_t)g * B, flags.data() + (size_t)g * B);
    }
  }
  if (g_times.on)
    std::cerr << "Timing: interval pairs: inputs and walks " << t_fit - t_start << " s, cells, rows and fits " << StageTimes::now() - t_fit
              << " s (device kernels " << kernel_s << " s); " << total_recs << " records uploaded" << std::endl;
  if (run.status) return run.status;
  print_usage_footer();
  return 0;
}

// `--mode mut_interval --pairs LIST`: the single run above for every line of the list, in one pass (fit_pair_list).
static int run_mut_interval_pairs(const Options& opt) {
  if (refuse_options(opt, {"target_tmp", "reference_tmp", "rows", "write_rows", "output", "ranks", "target_age", "reference_age"},
                     "--mode mut_interval --pairs") ||
      refuse_per_line_options(opt))
    return 1;
  if (!opt.has("mut")) {
    std::cerr << "Error: --pairs needs --mut (and optionally --chr, --bins, --num_bootstraps, --seed, --years_per_gen, --max_iter, "
                 "--min_iter, --device)."
              << std::endl;
    return 1;
  }
  std::vector<std::string> names, mut_files;
  chromosome_files(opt, names, mut_files);
  std::vector<PairSpec> pairs;
  if (!read_pair_list(opt.get("pairs"), opt, names, pairs)) return 1;
  for (const PairSpec& ps : pairs)
    if (ps.ages_given) {
      std::cerr << "Error: " << opt.get("pairs") << ", line " << ps.line
                << ": --mode mut_interval takes modern samples only: a line cannot carry sample ages." << std::endl;
      return 1;
    }
  if (!pairs_have_epochs(opt, pairs)) return 1;
  std::cerr << "---------------------------------------------------------" << std::endl;
  std::cerr << "Calculating coalescence rates from interval-dated mutations for " << pairs.size() << " pairs.." << std::endl;
  FitRun run(opt);
  if (!run.read_replicates(opt, true)) return 1;
  if (!fit_run_device(opt, run)) return 1;
  return fit_pair_list(opt, run, names, mut_files, pairs, nullptr);
}

// ------------------------------------------------------------------ `--mode mut_interval --samples LIST`
// (the list: read_sample_list, cli_lists.h; no ages here)
// Every (target line, reference line) of the list with different lines, targets outermost; each pair's PREFIX_<target>_<reference>.coal
// is, byte for byte, what `--pairs` writes for it given the expanded list.  Where every file has a walk index the pairs are not
// walked on the host at all: N index arrays and the rows go to the device once and colate_interval_fit_samples forms every pair's
// records where the cells kernel reads them (its host twin without a device or with COLATE_DEVICE_INTERVAL=0).  Otherwise, or with
// COLATE_DEVICE_INTERVAL_WALK=0, the expanded list takes the path of `--pairs` after one line on stderr.
static int run_mut_interval_samples(const Options& opt) {
  if (refuse_options(opt, {"pairs", "rows", "target_tmp", "reference_tmp", "write_rows", "target_mask", "reference_mask", "ranks", "target_age",
                           "reference_age"},
                     "--mode mut_interval --samples"))
    return 1;
  if (!opt.has("mut") || !opt.has("output") || (!opt.has("bins") && !opt.has("coal"))) {
    std::cerr << "Error: --samples needs --mut, -o PREFIX and --bins x,y,stepsize or --coal FILE (optional: --chr, --num_bootstraps, --seed, "
                 "--years_per_gen, --max_iter, --min_iter, --device)."
              << std::endl;
    return 1;
  }
  std::vector<std::string> names, mut_files;
  chromosome_files(opt, names, mut_files);
  std::vector<SampleLine> samples;
  if (!read_sample_list(opt.get("samples"), opt, names, false, samples)) return 1;
  std::vector<PairSpec> pairs;
  if (!sample_pairs(samples, opt.get("output"), opt.get("samples"), pairs)) return 1;
  const size_t P = pairs.size();
  std::cerr << "---------------------------------------------------------" << std::endl;
  std::cerr << "Calculating coalescence rates from interval-dated mutations for " << P << " pairs.." << std::endl;
  FitRun run(opt);
  if (!run.read_replicates(opt, true)) return 1;
  if (!fit_run_device(opt, run)) return 1;
  if (const char* e = std::getenv("COLATE_DEVICE_INTERVAL_WALK"))
    if (std::string(e) == "0") {
      std::cerr << "pairs walked on the host through the engine (COLATE_DEVICE_INTERVAL_WALK=0)" << std::endl;
      return fit_pair_list(opt, run, names, mut_files, pairs, nullptr);
    }
  const double t_start = StageTimes::now();
  WalkInputs in;
  if (!load_walk_inputs(names, mut_files, pairs, in)) return 1;
  if (!in.indexed) {
    std::cerr << "pairs walked on the host through the engine (a sample has no walk index)" << std::endl;
    return fit_pair_list(opt, run, names, mut_files, pairs, &in);
  }

  // ---- one set of epochs and starting rates for all pairs: --bins, else --coal
  std::vector<double> epochs, init;
  int ep_null = 0;
  if (!fit_run_epochs(opt, run, opt.has("bins") ? nullptr : &opt.get("coal"), "Error: ", epochs, init, ep_null)) return 1;
  const int E = (int)epochs.size();

  const bool on_host = !run.host_why.empty();
  std::cerr << in.S << " samples and " << in.M << " masks staged, " << P << " pairs walked on the " << (on_host ? "host" : "device")
            << std::endl;
  std::cerr << "Maximising likelihood using EM.. " << std::endl;
  if (on_host) std::cerr << "interval cells and fits on the host (" << run.host_why << ")" << std::endl;
  const colate_iw::View v = in.walk_view(kIntervalBasesPerBlock);
  const size_t PB = P * (size_t)run.B;
  std::vector<int> nb(P), R(P), iters(PB), flags(PB);
  std::vector<long long> used(P), dropped(P);
  std::vector<double> rates(PB * E), ll(PB);
  const colate_iw::FitArgs args{run.B,        E,           epochs.data(), init.data(),   (unsigned)run.seed, run.max_iter, run.min_iter,
                                COLATE_DEFAULT_REL_TOL, COLATE_DEFAULT_RATE_FLOOR, nb.data(), used.data(), R.data(), dropped.data(),
                                rates.data(), iters.data(), ll.data(), flags.data()};
  const double t_fit = StageTimes::now();
  if (int rc = on_host ? colate_iw::fit_samples_view_host(v, args, 1) : colate_iw::fit_samples_view_device(v, args)) return api_error(rc);
  long long total_recs = 0;
  for (size_t p = 0; p < P; p++) {
    total_recs += used[p];
    say_blocks(p, P, pairs[p], nb[p]);
    report_pair(run, p, pairs[p], R[p], dropped[p], E, epochs.data(), ep_null, rates.data() + p * run.B * E, iters.data() + p * run.B,
                flags.data() + p * run.B);
  }
  if (g_times.on)
    std::cerr << "Timing: interval samples: inputs " << t_fit - t_start << " s, walks, cells, rows and fits " << StageTimes::now() - t_fit
              << " s (device kernels " << (on_host ? 0.0 : colate_interval_fit_samples_kernel_seconds()) << " s); " << in.row_off.back()
              << " rows, " << in.S << " index arrays and " << in.M << " masks staged, " << total_recs << " records formed" << std::endl;
  if (run.status) return run.status;
  print_usage_footer();
  return 0;
}

int run_mut_interval(const Options& opt) {
  if (opt.has("samples")) return run_mut_interval_samples(opt);
  if (opt.has("pairs")) return run_mut_interval_pairs(opt);
  const bool from_mut = opt.has("mut") || opt.has("target_tmp") || opt.has("reference_tmp");
  if (from_mut && refuse_options(opt, {"rows"}, "--mut, --target_tmp or --reference_tmp")) return 1;
  if (from_mut && (opt.has("target_age") || opt.has("reference_age"))) {
    std::cerr << "Error: --mode mut_interval takes modern samples only: --target_age and --reference_age are not supported." << std::endl;
    return 1;
  }
  const bool inputs_ok = from_mut ? opt.has("mut") && opt.has("target_tmp") && opt.has("reference_tmp") : opt.has("rows");
  if (!inputs_ok || !opt.has("output") || (!opt.has("bins") && !opt.has("coal"))) {
    std::cerr << "Error: --mode mut_interval needs --rows FILE (or --mut, --target_tmp and --reference_tmp), -o OUT and --bins "
                 "x,y,stepsize or --coal FILE (optional: --chr, --target_mask, --reference_mask, --write_rows, --num_bootstraps, "
                 "--seed, --years_per_gen, --max_iter, --min_iter, --device)."
              << std::endl;
    return 1;
  }
  std::cerr << "---------------------------------------------------------" << std::endl;
  std::cerr << "Calculating coalescence rates from interval-dated mutations.." << std::endl;
  FitRun run(opt);
  if (!run.read_replicates(opt, true)) return 1;
  // ---- epochs and starting rates (--coal, else --bins; the library's message without a lead), then device or host twin
  std::vector<double> epochs, init_rates;
  int ep_null = 0;
  if (!fit_run_epochs(opt, run, opt.has("coal") ? &opt.get("coal") : nullptr, "", epochs, init_rates, ep_null)) return 1;
  const int E = (int)epochs.size();
  if (!fit_run_device(opt, run)) return 1;
  const int B = run.B, max_iter = run.max_iter, min_iter = run.min_iter;
  const std::string& host_why = run.host_why;

  // ---- the rows and the per-block tables
  IntervalRows rows;
  if (from_mut) {
    if (!rows_from_mut(opt, !host_why.empty(), host_why, rows)) return 1;
  } else {
    std::string err;
    if (!read_interval_rows(opt.get("rows"), epochs[0], rows, err)) {
      std::cerr << "Error: " << err << std::endl;
      return 1;
    }
    std::cerr << "Number of blocks: " << rows.nb << std::endl;
    std::cerr << "Number of rows: " << rows.R << std::endl;
  }
  const int nb = rows.nb, R = rows.R;
  if (opt.has("write_rows") && !write_interval_rows(opt.get("write_rows"), rows)) {
    std::cerr << "Error: cannot write " << opt.get("write_rows") << std::endl;
    return 1;
  }

  // ---- block weights (coal.cpp:3350-3357)
  std::mt19937 rng(run.seed);
  std::vector<double> weights((size_t)B * nb);
  if (int rc = colate_bootstrap_weights(&rng, B, nb, weights.data())) return api_error(rc);

  std::cerr << "Maximising likelihood using EM.. " << std::endl;
  std::vector<double> rates((size_t)B * E), ll(B);
  std::vector<int> iters(B), flags(B);
  if (!host_why.empty()) std::cerr << "interval fit on the host (" << host_why << ")" << std::endl;
  const int rc = host_why.empty()
                     ? colate_bootstrap_em_interval_batch(B, nb, R, E, rows.kinds.data(), rows.age_begin.data(), rows.age_end.data(),
                                                          weights.data(), rows.tables.data(), epochs.data(), init_rates.data(), max_iter,
                                                          min_iter, COLATE_DEFAULT_REL_TOL, COLATE_DEFAULT_RATE_FLOOR, rates.data(),
                                                          iters.data(), ll.data(), flags.data())
                     : colate_bootstrap_em_interval_batch_host(B, nb, R, E, rows.kinds.data(), rows.age_begin.data(), rows.age_end.data(),
                                                               weights.data(), rows.tables.data(), epochs.data(), init_rates.data(),
                                                               max_iter, min_iter, COLATE_DEFAULT_REL_TOL, COLATE_DEFAULT_RATE_FLOOR,
                                                               rates.data(), iters.data(), ll.data(), flags.data(), 1);
  if (rc) return api_error(rc);
  report_bootstraps(0, B, E, iters.data(), flags.data(), false);
  if (!write_coal(opt.get("output"), B, E, epochs.data(), rates.data(), false, ep_null)) return 1;
  print_usage_footer();
  return 0;
}

}  // namespace colate_drv
