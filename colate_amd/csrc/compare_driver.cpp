// colate_amd/csrc/compare_driver.cpp -- `Colate --mode compare_tmp` (compare_tmp.h: the contract, include/coal/coal.cpp:4297-4521):
// per 10 Mb window of every chromosome the SNPs at which both samples of a pair have data and how many of them the two
// disagree on.
//   * `--target_tmp T --reference_tmp R --mut P -o OUT [--chr FILE] [--seed S]`: the reference's single run, OUT byte for byte
//     its file.  The cursor walk on the host; no device is opened (one pair is a pass over two arrays).  --seed is accepted and
//     has no effect: the reference's draws decide nothing.  COLATE_DEVICE_COMPARE=1 sends the pair through the indexed path
//     below as a list of one pair.
//   * `--samples LIST --mut P -o PREFIX [--chr FILE] [--device D]`: every (target line, reference line) of the list on different
//     lines, targets outermost; PREFIX_<target>_<reference>.txt is the single run's file, PREFIX.pairs.txt holds one line
//     `target reference mismatch snps` per pair, the integer totals.  The rows and one walk index per sample are staged once
//     and colate_compare_samples counts every pair on the device; its host twin without a device or with
//     COLATE_DEVICE_COMPARE=0; the cursor walk per pair where a sample has no walk index or the raw rows of a .mut file
//     descend.  All three give the same bytes.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include "cli_lists.h"
#include "cli_modes.h"
#include "colate_amd.h"
#include "compare_tmp.h"
#include "walk_inputs.h"

namespace colate_drv {

namespace {

// One pair's file: a line per window, `name current_bp num_mismatch num_snps`, the counts written as the doubles they are in
// the reference (a count of 1 000 000 prints as 1e+06).
bool write_windows(const std::string& path, const std::vector<std::string>& names, const std::vector<CompareChromosome>& chr,
                   const int* mismatch, const int* snps) {
  std::ofstream os(path);
  size_t at = 0;
  for (size_t c = 0; c < names.size(); c++)
    for (int w = 0; w < chr[c].windows; w++, at++)
      os << names[c] << " " << (int)((long long)chr[c].first_pos + (long long)w * colate_cmp::kBinSize) << " " << (double)mismatch[at] << " "
         << (double)snps[at] << "\n";
  return close_checked(os, path);
}

double g_pair_stage_s = 0;  // the seconds of the pair stage alone, whichever form ran (COLATE_TIMING)

// Loads the inputs of `pairs` and counts every pair: mismatch / snps [P][sum of windows].  False after an error message;
// nothing has been written then.
bool count_pairs(const Options& opt, const std::vector<std::string>& names, const std::vector<std::string>& mut_files,
                 const std::vector<PairSpec>& pairs, Path want, WalkInputs& in, std::vector<int>& mismatch, std::vector<int>& snps) {
  std::vector<const std::string*> files;
  for (const PairSpec& ps : pairs) files.insert(files.end(), {&ps.target, &ps.reference});
  if (!check_readable(files, "cannot open")) return false;
  if (!load_walk_inputs(names, mut_files, pairs, in, RowSet::compare_tmp)) return false;
  if (!in.files_ok) {
    std::cerr << "Error: a .colate.in file could not be read." << std::endl;
    return false;
  }
  for (size_t c = 0; c < names.size(); c++)
    if (in.compare[c].raw_rows == 0) {
      std::cerr << "Error: " << mut_files[c] << " has no rows." << std::endl;
      return false;
    }
  const size_t P = pairs.size();
  if (want != Path::cursors && !in.indexed) {
    std::cerr << "pairs compared on the host through the record cursors (a sample has no walk index, or the rows of a .mut file descend)"
              << std::endl;
    want = Path::cursors;
  }
  const double t_stage = StageTimes::now();
  if (want == Path::cursors) {
    const bool ok = compare_cursor_pairs(in, names, pairs, mismatch, snps);
    g_pair_stage_s = StageTimes::now() - t_stage;
    return ok;
  }
  const int C = (int)names.size();
  std::vector<int> first((size_t)C), last((size_t)C);
  long long Wt = 0;
  for (int c = 0; c < C; c++) first[(size_t)c] = in.compare[(size_t)c].first_pos, last[(size_t)c] = in.compare[(size_t)c].last_pos, Wt += in.compare[(size_t)c].windows;
  colate_cmp::View v;
  v.C = C, v.row_off = in.row_off.data(), v.rows = in.row_ptrs.data(), v.S = in.S, v.idx = in.idx_ptrs.data(), v.P = (int)P;
  v.pairs = in.pairs.data(), v.first_pos = first.data(), v.last_pos = last.data(), v.window = colate_cmp::kBinSize;
  mismatch.assign(P * (size_t)Wt, 0), snps.assign(P * (size_t)Wt, 0);
  std::vector<long long> win_off((size_t)C + 1);
  if (want == Path::device && !bind_device(opt)) return false;
  const long long cap = (long long)P * Wt;
  if (int rc = want == Path::device ? colate_cmp::compare_view_device(v, cap, win_off.data(), mismatch.data(), snps.data())
                                    : colate_cmp::compare_view_host(v, cap, win_off.data(), mismatch.data(), snps.data()))
    return api_error(rc), false;
  g_pair_stage_s = StageTimes::now() - t_stage;
  if (win_off[(size_t)C] != Wt) {  // (the loader's window loop and window_of agree where the raw rows do not descend)
    std::cerr << "Error: the windows of the indexed form (" << win_off[(size_t)C] << ") are not those of the rows (" << Wt << ")." << std::endl;
    return false;
  }
  std::cerr << in.S << " samples staged, " << P << " pairs compared on the " << (want == Path::device ? "device" : "host") << std::endl;
  return true;
}

int run_compare_samples(const Options& opt) {
  if (refuse_options(opt, {"pairs", "target_tmp", "reference_tmp", "target_mask", "reference_mask", "target_age", "reference_age", "bins", "coal",
                           "num_bootstraps", "ranks", "devices"},
                     "--mode compare_tmp --samples"))
    return 1;
  if (!opt.has("mut") || !opt.has("output")) {
    std::cerr << "Error: --samples needs --mut and -o PREFIX (optional: --chr, --seed, --device)." << std::endl;
    return 1;
  }
  std::vector<std::string> names, mut_files;
  chromosome_files(opt, names, mut_files);
  std::vector<SampleLine> samples;
  if (!read_sample_list(opt.get("samples"), opt, names, false, samples)) return 1;
  for (const SampleLine& sl : samples)
    if (!sl.masks.empty()) {
      std::cerr << "Error: " << opt.get("samples") << ", line " << sl.line << ": mask= is not supported by --mode compare_tmp" << std::endl;
      return 1;
    }
  std::vector<PairSpec> pairs;
  if (!sample_pairs(samples, opt.get("output"), opt.get("samples"), pairs)) return 1;
  for (PairSpec& ps : pairs) ps.output += ".txt";
  std::cerr << "---------------------------------------------------------" << std::endl;
  std::cerr << "Comparing Colate tmp input files for " << pairs.size() << " pairs.." << std::endl;
  std::string why;
  const Path want = choose_path("COLATE_DEVICE_COMPARE", true, why);
  if (want != Path::device) std::cerr << "pairs compared on the host (" << why << ")" << std::endl;
  const double t0 = StageTimes::now();
  WalkInputs in;
  std::vector<int> mismatch, snps;
  if (!count_pairs(opt, names, mut_files, pairs, want, in, mismatch, snps)) return 1;
  const double t1 = StageTimes::now();
  const size_t Wt = mismatch.size() / pairs.size();
  std::ofstream os(opt.get("output") + ".pairs.txt");
  for (size_t p = 0; p < pairs.size(); p++) {
    if (!write_windows(pairs[p].output, names, in.compare, mismatch.data() + p * Wt, snps.data() + p * Wt)) return 1;
    long long mm = 0, n = 0;
    for (size_t w = 0; w < Wt; w++) mm += mismatch[p * Wt + w], n += snps[p * Wt + w];
    os << pairs[p].target_name << " " << pairs[p].ref_name << " " << mm << " " << n << "\n";
  }
  if (!close_checked(os, opt.get("output") + ".pairs.txt")) return 1;
  if (g_times.on)
    std::cerr << "Timing: compare samples: inputs " << t1 - t0 - g_pair_stage_s << " s, pair stage " << g_pair_stage_s << " s (device kernels "
              << colate_compare_samples_kernel_seconds() << " s), files " << StageTimes::now() - t1 << " s; " << (in.row_off.empty() ? 0LL : in.row_off.back()) << " rows, "
              << in.S << " index arrays, " << pairs.size() << " pairs, " << Wt << " windows" << std::endl;
  print_usage_footer();
  return 0;
}

}  // namespace

int run_compare_tmp(const Options& opt) {
  if (opt.has("samples")) return run_compare_samples(opt);
  if (!opt.has("target_tmp") || !opt.has("reference_tmp") || !opt.has("mut") || !opt.has("output") || opt.has("help")) {  // coal.cpp:4302-4312
    if (!opt.has("help")) {
      std::cout << "Not enough arguments supplied." << std::endl;
      std::cout << "Needed: target_tmp, reference_tmp, mut, output. Optional: chr." << std::endl;
    }
    print_help();
    std::cout << "Compare tmp." << std::endl;
    return 0;
  }
  std::cerr << "---------------------------------------------------------" << std::endl;
  std::cerr << "Calculating Colate tmp input file for " << opt.get("target_tmp") << ".." << std::endl;
  if (opt.has("seed")) (void)opt.get_int("seed");  // (read as the reference reads it; the draws decide nothing)
  std::vector<std::string> names, mut_files;
  chromosome_files(opt, names, mut_files);
  PairSpec ps;
  ps.target = opt.get("target_tmp"), ps.reference = opt.get("reference_tmp"), ps.output = opt.get("output");
  std::string why;
  const Path want = choose_path("COLATE_DEVICE_COMPARE", false, why);
  WalkInputs in;
  std::vector<int> mismatch, snps;
  if (!count_pairs(opt, names, mut_files, std::vector<PairSpec>(1, ps), want, in, mismatch, snps)) return 1;
  if (!write_windows(ps.output, names, in.compare, mismatch.data(), snps.data())) return 1;
  print_usage_footer();
  return 0;
}

}  // namespace colate_drv
