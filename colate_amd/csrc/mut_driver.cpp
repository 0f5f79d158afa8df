// colate_amd/csrc/mut_driver.cpp -- `Colate` as a library call (colate_mut_main in include/colate_amd.h): the command line of
// the reference (include/coal/Colate.cpp:6-116), the table of its modes, and `--mode mut`: the mut() driver
// (include/coal/coal.cpp:3071-3863) around the GPU EM (colate_em_batch), for one pair (run_mut), for a `--pairs` list
// (run_mut_pairs; the tables of both come from the engine of mut_pairs.cpp) and for the pairs of a `--samples` list
// (run_mut_samples; the tables come from the walk and fill on the device, fill_samples.cpp).  The two lists share run_pair_list,
// everything behind the fill.  The readers are in mut_readers.cpp, what the modes share around their lists and per-pair runs in
// cli_lists.cpp, the `--ranks` launcher in mut_ranks.cpp, `--mode make_tmp` in make_tmp.cpp.
//
// Everything here runs once per invocation on the host; the per-replicate EM,
// which is where the reference spends its time, is the HIP kernel.
#include <sys/resource.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <functional>
#include <iomanip>
#include <iostream>
#include <sstream>
#include <thread>

#include "cli_lists.h"
#include "cli_modes.h"
#include "colate_amd.h"
#include "colate_internal.h"
#include "rank_ctx.h"

namespace colate_drv {

// ------------------------------------------------------------------ options
// Same option names as Colate.cpp:11-45 (unknown options are an error there too:
// cxxopts throws option_not_exists_exception).  `--num_bootstrap` (README spelling)
// is accepted as an alias of `--num_bootstraps`.  Ours: `--device N` (GPU ordinal), `--devices N`
// (shard the replicates over GPUs 0..N-1 of the node from this one process), `--ranks N` (the same sharding as N
// processes, one per GPU, with one RCCL all-gather of the results: run_ranked below),
// `--counts_out FILE` (write the bootstrap count tables in the reference's .colate_mat layout,
// 17 significant digits), `--counts_only` (stop after that; needs no GPU) and `--write_colate_mat` (write
// <output>.colate_mat exactly as the reference does for BCF/BAM inputs, coal.cpp:3336-3343, 3453-3470).

const char* const kValueOptions[] = {
    "mode", "anc", "mut", "target_bcf", "reference_bcf", "target_mask", "reference_mask",
    "target_table", "target_bam", "reference_bam", "target_tmp", "reference_tmp", "target_age",
    "reference_age", "ref_genome", "anc_genome", "mask", "mask_cutoff", "chr", "bins",
    "lineage_bin", "outgroup_tmrca", "years_per_gen", "coal", "seed", "num_bootstraps", "filters",
    "groups", "poplabels", "map", "input", "output", "device", "devices", "ranks", "counts_out", "pairs",
    "rows", "max_iter", "min_iter", "write_rows", "samples", "age_profile", "block_bases"};
const char* const kBoolOptions[] = {"help", "strandfilter", "counts_only", "write_colate_mat", "profile_only", "jackknife", "expected"};

bool parse_options(int argc, char** argv, Options& o, std::string& err) {
  for (int i = 1; i < argc; i++) {
    std::string a = argv[i];
    std::string name, value;
    bool have_value = false;
    if (a.rfind("--", 0) == 0) {
      name = a.substr(2);
      size_t eq = name.find('=');
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
    if (name == "num_bootstrap") name = "num_bootstraps";
    bool is_bool = false, known = false;
    for (const char* b : kBoolOptions)
      if (name == b) is_bool = known = true;
    for (const char* v : kValueOptions)
      if (name == v) known = true;
    if (!known) {
      err = "Option '" + name + "' does not exist";
      return false;
    }
    if (is_bool) {
      o.kv[name] = "true";
      continue;
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

void print_help() {
  std::cout << "Usage:\n  Colate [OPTION...]\n\n"
            << "      --help                 Print help.\n"
            << "      --mode arg             Choose which part of the algorithm to run (colate_amd: mut, mut_interval, compare_tmp, count_topo, make_tmp, CondCoalRates).\n"
            << "      --mut arg              Filename of file containing mut.\n"
            << "      --target_tmp arg       Filename of target tmp file\n"
            << "      --reference_tmp arg    Filename of reference tmp file\n"
            << "      --target_mask arg      Fasta file containing target mask\n"
            << "      --reference_mask arg   Fasta file containing reference mask\n"
            << "      --target_age arg       Target age in years\n"
            << "      --reference_age arg    Reference age in years\n"
            << "      --chr arg              Optional: File specifying chromosomes to use.\n"
            << "      --bins arg             Optional: Epoch boundaries 10^(seq(x,y,stepsize)) [format: x,y,stepsize]. In years.\n"
            << "      --years_per_gen arg    Optional: Years per generation.\n"
            << "      --coal arg             Filename of file containing coalescence rates.\n"
            << "      --seed arg             Optional: Seed for random number generator (int)\n"
            << "      --num_bootstraps arg   Optional: Number of bootstraps.\n"
            << "      --device arg           Optional (colate_amd): GPU ordinal, default 0.\n"
            << "      --devices arg          Optional (colate_amd): shard the bootstrap replicates over GPUs 0..N-1 (one process).\n"
            << "      --ranks arg            Optional (colate_amd): the same as N processes, one per GPU, one RCCL all-gather.\n"
            << "      --pairs arg            Optional (colate_amd): file of `target_tmp reference_tmp output [target_age [reference_age]]`\n"
            << "                             lines; all pairs share --mut/--chr/--bins/--num_bootstraps/--seed, each .mut is parsed\n"
            << "                             once and all replicates of all pairs run in one GPU launch.  After the three names a\n"
            << "                             line may carry, in any order and mixed with the ages, target_mask=PREFIX,\n"
            << "                             reference_mask=PREFIX (expanded as --target_mask / --reference_mask are) and\n"
            << "                             coal=FILE (the pair's --coal warm start; --bins is then not needed for that line).\n"
            << "                             (--mode mut_interval) --pairs FILE with --mut [--chr, --bins]: the same lines without ages;\n"
            << "                             every pair's interval-dated fit in one pass, each <output>.coal that of its single run.\n"
            << "      --samples arg          (--mode mut_interval) file of `NAME FILE.colate.in [mask=PREFIX] [role=target|reference]`\n"
            << "                             lines; with --mut, -o PREFIX [--chr] and --bins or --coal every target x reference pair of\n"
            << "                             different lines is fitted, the pairs walked on the GPU; writes PREFIX_<target>_<reference>.coal,\n"
            << "                             each the file `--pairs` writes for that pair.\n"
            << "                             (--mode mut) the same list, a line may add age=YEARS; the pairs are walked and their tables\n"
            << "                             filled on the GPU; PREFIX_<target>_<reference>.coal (and .counts) as `--mode mut --pairs` writes them.\n"
            << "                             (--mode compare_tmp) the same list without mask= and age=; with --mut and -o PREFIX every pair's\n"
            << "                             windowed mismatch counts, compared on the GPU: PREFIX_<target>_<reference>.txt and PREFIX.pairs.txt.\n"
            << "                             (--mode count_topo) that list with role= a comma-separated subset of cond,target,reference (default: all\n"
            << "                             three); every (cond, target, reference) of three lines, drawn on the GPU: PREFIX_<cond>_<target>_<reference>.txt\n"
            << "                             and PREFIX.triples.txt.\n"
            << "      --age_profile arg      (--mode count_topo --samples) x,y,stepsize as for --bins [--years_per_gen, default 28]: also write\n"
            << "                             PREFIX.profile.txt, `cond target reference epoch plus minus qualifying` per (triple, epoch): the\n"
            << "                             printed rows of either sign and the rows that drew, binned on the GPU by the mid of their ages.\n"
            << "      --profile_only         (--mode count_topo --samples --age_profile) write no per-triple file: PREFIX.profile.txt and\n"
            << "                             PREFIX.triples.txt only.\n"
            << "      --jackknife            (--mode count_topo --samples --age_profile) also write PREFIX.jackknife.txt, `cond target reference\n"
            << "                             epoch plus minus blocks D D_jack se Z` per (triple, epoch) and for epoch `all`: the delete-one block\n"
            << "                             jackknife of (plus - minus) / (plus + minus) over genome blocks, counted per block on the GPU.\n"
            << "      --block_bases arg      (--jackknife) bases per genome block, an integer of at least 1 (default 30000000).\n"
            << "      --expected             (--mode count_topo --samples --age_profile) write PREFIX.expected.txt in place of every sampled file:\n"
            << "                             per (triple, epoch) the expected plus and minus given the read counts, summed on the GPU in units\n"
            << "                             of 2^-30; no draws, --seed has no effect.  With --jackknife also PREFIX.expected.jackknife.txt.\n"
            << "      --counts_out arg       Optional (colate_amd): write the bootstrap count tables (.colate_mat layout).\n"
            << "      --counts_only          Optional (colate_amd): stop after --counts_out (no GPU needed).\n"
            << "      --write_colate_mat     Optional (colate_amd): write <output>.colate_mat as the reference does for BCF/BAM inputs.\n"
            << "      --target_table arg     (--mode make_tmp) Table `chr bp allele` of the target's calls.\n"
            << "      --ref_genome arg       (--mode make_tmp) Reference genome fasta (per chromosome with --chr).\n"
            << "      --input arg            (--mode CondCoalRates) Prefix of the Relate .anc / .mut files.\n"
            << "      --poplabels arg        (--mode CondCoalRates) Poplabels file (groups: its second column).\n"
            << "      --groups arg           (--mode CondCoalRates) FOCAL,CONDITIONAL group names.\n"
            << "      --lineage_bin arg      (--mode CondCoalRates) log10 of the focal epoch boundary in years (default 1e5).\n"
            << "      --mask arg             (--mode CondCoalRates) Fasta mask (per chromosome with --chr).\n"
            << "                             (--mode CondCoalRates) --pairs FILE: `FOCAL,CONDITIONAL OUTPUT` per line, in place of\n"
            << "                             --groups / --output; every table is its single run's, from one pass over the trees.\n"
            << "      --rows arg             (--mode mut_interval) File of `block kind age_begin age_end weight` lines (plain or gzip):\n"
            << "                             block a non-negative integer, kind shared|notshared, ages in generations; with --bins or\n"
            << "                             --coal, --num_bootstraps, --seed, --years_per_gen; writes <output>.coal.\n"
            << "                             (--mode mut_interval) or --mut, --target_tmp, --reference_tmp [--chr, --target_mask,\n"
            << "                             --reference_mask] as for --mode mut: every used SNP is one interval-dated observation.\n"
            << "      --write_rows arg       (--mode mut_interval) Write the rows and per-block weights in the --rows format.\n"
            << "      --max_iter arg         (--mode mut_interval) Iteration cap of the EM (default 100000).\n"
            << "      --min_iter arg         (--mode mut_interval) Iterations before the stop rule applies (default 1000).\n"
            << "  -o, --output arg           Filename of output.\n"
            << std::endl;
}

void print_usage_footer() {  // coal.cpp:3852-3861
  rusage usage;
  getrusage(RUSAGE_SELF, &usage);
  std::cerr << "CPU Time spent: " << usage.ru_utime.tv_sec << "." << std::setfill('0') << std::setw(6)
            << usage.ru_utime.tv_usec << "s; Max Memory usage: " << usage.ru_maxrss / 1000.0 << "Mb." << std::endl;
  std::cerr << "---------------------------------------------------------" << std::endl << std::endl;
}

int api_error(int rc) {
  std::cerr << "Error: " << colate_last_error() << " (" << rc << ")" << std::endl;
  return 1;
}

// ------------------------------------------------------------------ what the single-pair and the list drivers of `--mode mut` share
namespace {

// OUT.colate_mat (coal.cpp:3471-3499): 185 grid values, then per replicate 185 shared
// and 185 not-shared counts, read with operator>> (a failed extraction leaves zeros).
bool load_colate_mat(const std::string& path, int B, int A, std::vector<double>& grid,
                     std::vector<double>& csh, std::vector<double>& cns) {
  GzText is;
  if (!is.open(path)) return false;
  std::istringstream ss(is.read_all());
  for (int b = 0; b < A; b++) ss >> grid[b];
  csh.assign((size_t)B * A, 0.0);
  cns.assign((size_t)B * A, 0.0);
  for (int i = 0; i < B; i++) {
    for (int b = 0; b < A; b++) ss >> csh[(size_t)i * A + b];
    for (int b = 0; b < A; b++) ss >> cns[(size_t)i * A + b];
  }
  return true;
}

void write_counts_file(const std::string& path, int B, int A, const std::vector<double>& grid,
                       const double* csh, const double* cns) {
  FILE* f = std::fopen(path.c_str(), "w");
  if (!f) {
    std::cerr << "Error: cannot write " << path << std::endl;
    std::exit(1);
  }
  for (int b = 0; b < A; b++) std::fprintf(f, "%.17g ", grid[b]);
  std::fprintf(f, "\n");
  for (int i = 0; i < B; i++) {
    for (int b = 0; b < A; b++) std::fprintf(f, "%.17g ", csh[(size_t)i * A + b]);
    std::fprintf(f, "\n");
    for (int b = 0; b < A; b++) std::fprintf(f, "%.17g ", cns[(size_t)i * A + b]);
    std::fprintf(f, "\n");
  }
  std::fclose(f);
}

// the age grid of the A bins that every pair of a run shares
std::vector<double> shared_age_grid() {
  std::vector<double> grid(256);
  grid.resize(colate_age_grid(grid.data(), 256));
  return grid;
}

// One process, one GPU: create the HIP context on a second thread while this one reads the inputs (a fresh process pays a
// few hundred ms for it; end to end 0.63 -> see profiles/r02/bench/e2e.txt); joined when the guard goes.  Not with --ranks
// (every rank picks its own device after the fork) or --devices (several contexts), not when no device is needed.
struct DeviceWarmUp {
  std::thread t;
  explicit DeviceWarmUp(const Options& opt) {
    if (g_rank.ranked || opt.has("devices") || opt.has("counts_only")) return;
    int dev = 0;  // the device the run will use (--device N)
    try {
      if (opt.has("device")) dev = opt.get_int("device");
    } catch (...) {
      dev = 0;  // (reported where the option is used)
    }
    t = std::thread([dev] { (void)colate_warm_up(dev); });
  }
  ~DeviceWarmUp() {
    if (t.joinable()) t.join();
  }
};

// --device N: this process's GPU (a rank picks its own, RankComm); --devices N: `devs` = 0..N-1 to shard the rows over
// (left empty without it).  False after the error message.
bool bind_devices(const Options& opt, std::vector<int>& devs) {
  if (!g_rank.ranked && !bind_device(opt)) return false;
  if (opt.has("devices")) {
    const int nd = opt.get_int("devices");
    if (nd < 1) {
      std::cerr << "Error: --devices must be at least 1." << std::endl;
      return false;
    }
    for (int d = 0; d < nd; d++) devs.push_back(d);
  }
  return true;
}

}  // namespace

int run_mut(const Options& opt) {
  if (!opt.has("mut") || !opt.has("output")) {  // coal.cpp:3077-3087
    std::cout << "Not enough arguments supplied." << std::endl;
    std::cout << "Needed: mut, bins, output. Optional: target_tmp, reference_tmp, target_age, "
                 "reference_age, target_mask, reference_mask, coal, num_bootstrap."
              << std::endl;
    print_help();
    return 0;
  }
  std::cerr << "---------------------------------------------------------" << std::endl;
  std::cerr << "Calculating coalescence rates for (ancient) samples.." << std::endl;
  const DeviceWarmUp warm(opt);

  double target_age = 0, ref_age = 0;
  try {
    if (opt.has("target_age")) target_age = opt.get_float("target_age");
    if (opt.has("reference_age")) ref_age = opt.get_float("reference_age");
  } catch (...) {
    std::cerr << "Error: sample ages must be numbers." << std::endl;
    return 1;
  }
  if (!(target_age >= 0.0) || !(ref_age >= 0.0)) {
    std::cerr << "Error: sample ages must be non-negative." << std::endl;
    return 1;
  }
  RunOptions run(opt);
  const double age = std::max(target_age, ref_age) / run.years_per_gen;
  std::cerr << age << std::endl;
  const bool is_ancient = age > 0.0;

  const double C = 10;
  std::vector<double> age_grid = shared_age_grid();
  const int A = (int)age_grid.size();
  std::cerr << "num_bins: " << A << std::endl;
  if (!run.read_replicates(opt, false)) return 1;
  const int num_bases_per_block = 30e6, seed = run.seed, B = run.B;
  std::mt19937 rng(seed);
  const std::string out = opt.get("output");

  std::vector<double> csh, cns, weights;
  PairTables tab;  // (block bootstrap + F redistribution, coal.cpp:3326-3451, on its flat [nb][A] tables)
  int num_blocks = 0;
  bool gpu_bootstrap = false;
  const std::string mat = out + ".colate_mat";
  if (std::ifstream(mat).good()) {  // coal.cpp:3169-3170, 3471-3499
    std::cerr << "Loading precomputed file " << mat << std::endl;
    load_colate_mat(mat, B, A, age_grid, csh, cns);
  } else if (opt.has("target_tmp") && opt.has("reference_tmp")) {
    std::vector<std::string> names, mut_files;
    std::vector<PairSpec> one(1);
    PairSpec& pair = one[0];
    pair.target = opt.get("target_tmp"), pair.reference = opt.get("reference_tmp");
    chromosome_files(opt, names, mut_files, &pair.target_masks, &pair.ref_masks);
    // The pair goes through the engine of the batched front end (mut_pairs.cpp) as a list of one: every .mut file parsed in
    // parallel, the .colate.in files mapped, the SNP walk on one thread and the age sampling of the genome blocks on all the
    // others (or on the GPU), exact table-driven age bins -- the same tables bit for bit (22 x 1M rows: 3.3 -> 0.x s of table
    // fill, profiles/r04/bench/e2e_large.txt).  COLATE_THREADS=1: the sequential feeder, which is also what the engine falls
    // back to.
    const char* thr_env = std::getenv("COLATE_THREADS");
    if (thr_env && std::atoi(thr_env) <= 1) {
      fill_tables_from_tmp(names, mut_files, pair.target, pair.reference, pair.target_masks, pair.ref_masks, C, rng,
                           num_bases_per_block, A, tab);
    } else {
      for (size_t chr = 0; chr < mut_files.size(); chr++) std::cerr << "parsing CHR: " << chr + 1 << " / " << mut_files.size() << std::endl;
      std::vector<PairTables> tabs;
      fill_pairs(opt, names, mut_files, one, {0}, seed, A, tabs);
      tab = std::move(tabs[0]);
      rng = tab.rng;
    }
    const int nb = tab.nb;
    std::cerr << "Number of blocks: " << nb << std::endl;
    if (nb < 1) {
      std::cerr << "Error: no genome blocks were read." << std::endl;
      return 1;
    }
    num_blocks = nb;
    csh.assign((size_t)B * A, 0.0);
    cns.assign((size_t)B * A, 0.0);
    // the weights come from the run's mt19937 either way (coal.cpp:3350-3357); the weighted sums and
    // the F redistribution run on the GPU together with the EM unless only the counts are wanted
    // (--counts_only, no device needed) or the replicates are sharded over several GPUs
    gpu_bootstrap = !opt.has("counts_only") && !opt.has("devices") && !(g_rank.ranked && opt.has("counts_out")) &&
                    !opt.has("write_colate_mat");
    if (gpu_bootstrap) {
      weights.resize((size_t)B * nb);
      if (int rc = colate_bootstrap_weights(&rng, B, nb, weights.data())) return api_error(rc);
    } else if (int rc = colate_bootstrap_counts(&rng, B, nb, A, age_grid.data(), age, tab.sh.data(), tab.ns.data(),
                                                tab.she.data(), tab.nse.data(), csh.data(), cns.data())) {
      return api_error(rc);
    }
  } else {
    std::cerr << "Error: colate_amd reads --target_tmp/--reference_tmp (.colate.in) inputs or an "
                 "existing <output>.colate_mat; BCF/BAM inputs go through `Colate --mode make_tmp` first."
              << std::endl;
    return 1;
  }

  auto write_counts = [&]() {  // same layout as the reference's .colate_mat (coal.cpp:3336-3343, 3453-3469)
    write_counts_file(opt.get("counts_out"), B, A, age_grid, csh.data(), cns.data());
  };
  if (opt.has("write_colate_mat") && num_blocks > 0) {
    // coal.cpp:3336-3343, 3453-3470 (what the reference does when its inputs are BCF/BAM files): the counts are divided
    // by 1e3 IN PLACE -- the EM then runs on the scaled tables -- and written with the stream's default 6 significant
    // digits: grid line, then per replicate a line of shared and a line of not-shared counts.  The file is what a later
    // run (ours or the reference's) picks up as "precomputed file" (coal.cpp:3471-3499).
    const double norm = 1e3;
    for (double& v : csh) v /= norm;
    for (double& v : cns) v /= norm;
    if (g_rank.rank == 0) {
      std::ofstream os_mat(mat);
      for (int b = 0; b < A; b++) os_mat << age_grid[b] << " ";
      os_mat << "\n";
      for (int i = 0; i < B; i++) {
        for (int b = 0; b < A; b++) os_mat << csh[(size_t)i * A + b] << " ";
        os_mat << "\n";
        for (int b = 0; b < A; b++) os_mat << cns[(size_t)i * A + b] << " ";
        os_mat << "\n";
      }
    }
  }
  if (opt.has("counts_out") && !gpu_bootstrap) {
    if (g_rank.rank == 0) write_counts();
  }
  auto report_times = [&]() {
    if (g_times.on)
      std::cerr << "Timing: parse_mut " << g_times.parse_mut << " s, table_fill " << g_times.table_fill << " s, bootstrap_em "
                << g_times.bootstrap_em << " s" << std::endl;
  };
  if (opt.has("counts_only")) {
    report_times();
    return 0;
  }

  // ---- epochs (coal.cpp:3501-3646)
  if (!opt.has("coal") && !opt.has("bins")) {
    std::cerr << "Error: need --bins or --coal." << std::endl;
    return 1;
  }
  std::vector<double> epochs, init_rates;
  int ep_null = 0;
  const int E = epochs_for(opt, opt.has("coal") ? &opt.get("coal") : nullptr, age, run.years_per_gen, epochs, init_rates, ep_null);
  if (E <= 0) {
    std::cerr << colate_last_error() << std::endl;
    return 1;
  }
  if (opt.has("coal")) {
    for (double r : init_rates) std::cerr << r << " ";
    std::cerr << std::endl;
  }

  std::cerr << "Maximising likelihood using EM.. " << std::endl;
  std::vector<int> devs;
  if (!bind_devices(opt, devs)) return 1;
  std::vector<double> rates((size_t)B * E), ll(B);
  std::vector<int> iters(B), flags(B);
  int rc;
  const double t_em0 = StageTimes::now();
  if (g_rank.ranked) {
    // one process per GPU: this rank's contiguous replicate range on its own device, then ONE RCCL all-gather
    RankComm comm;
    if (!comm.open(opt)) return 1;
    if (gpu_bootstrap)
      rc = colate_bootstrap_em_batch_allgather(comm.comm, B, num_blocks, E, A, age_grid.data(), age, weights.data(), tab.sh.data(),
                                               tab.ns.data(), tab.she.data(), tab.nse.data(), epochs.data(), init_rates.data(),
                                               COLATE_DEFAULT_MAX_ITER, COLATE_DEFAULT_MIN_ITER, COLATE_DEFAULT_REL_TOL,
                                               COLATE_DEFAULT_RATE_FLOOR, rates.data(), iters.data(), ll.data(), flags.data());
    else
      rc = colate_em_batch_allgather(comm.comm, B, E, A, age_grid.data(), csh.data(), cns.data(), epochs.data(),
                                     init_rates.data(), COLATE_DEFAULT_MAX_ITER, COLATE_DEFAULT_MIN_ITER,
                                     COLATE_DEFAULT_REL_TOL, COLATE_DEFAULT_RATE_FLOOR, rates.data(), iters.data(),
                                     ll.data(), flags.data());
    if (rc) return api_error(rc);
    if (g_rank.rank != 0) return 0;  // every rank holds all results; rank 0 reports and writes them
  } else if (!devs.empty()) {
    rc = colate_em_batch_sharded((int)devs.size(), devs.data(), B, E, A, age_grid.data(), csh.data(), cns.data(),
                                 epochs.data(), init_rates.data(), COLATE_DEFAULT_MAX_ITER,
                                 COLATE_DEFAULT_MIN_ITER, COLATE_DEFAULT_REL_TOL, COLATE_DEFAULT_RATE_FLOOR,
                                 rates.data(), iters.data(), ll.data(), flags.data());
  } else if (gpu_bootstrap) {
    rc = colate_bootstrap_em_batch(B, num_blocks, E, A, age_grid.data(), age, weights.data(), tab.sh.data(), tab.ns.data(),
                                   tab.she.data(), tab.nse.data(), epochs.data(), init_rates.data(), COLATE_DEFAULT_MAX_ITER,
                                   COLATE_DEFAULT_MIN_ITER, COLATE_DEFAULT_REL_TOL, COLATE_DEFAULT_RATE_FLOOR,
                                   rates.data(), iters.data(), ll.data(), flags.data(), csh.data(), cns.data());
    if (rc == 0 && opt.has("counts_out")) write_counts();
  } else {
    rc = colate_em_batch(B, E, A, age_grid.data(), csh.data(), cns.data(), epochs.data(),
                         init_rates.data(), COLATE_DEFAULT_MAX_ITER, COLATE_DEFAULT_MIN_ITER,
                         COLATE_DEFAULT_REL_TOL, COLATE_DEFAULT_RATE_FLOOR, rates.data(),
                         iters.data(), ll.data(), flags.data());
  }
  g_times.bootstrap_em = StageTimes::now() - t_em0;
  report_times();
  if (rc) return api_error(rc);
  report_bootstraps(0, B, E, iters.data(), flags.data(), true);
  if (!write_coal(out, B, E, epochs.data(), rates.data(), is_ancient, ep_null)) return 1;

  print_usage_footer();
  return 0;
}

// Everything of a run over a list of pairs but the list and the table fill: epochs per pair, classes by number of epochs,
// bootstrap weights from each pair's generator, counts, the EM launches and the writers.  fill(todo, seed, A, tabs): the tables
// of the pairs listed in `todo` and each one's generator after its fill, as fill_pairs leaves them.
using PairListFill = std::function<bool(const std::vector<size_t>& todo, int seed, int A, std::vector<PairTables>& tabs)>;
int run_pair_list(const Options& opt, const std::vector<PairSpec>& pairs, const PairListFill& fill) {
  const bool talk = g_rank.rank == 0;
  if (talk) {
    std::cerr << "---------------------------------------------------------" << std::endl;
    std::cerr << "Calculating coalescence rates for " << pairs.size() << " pairs of (ancient) samples.." << std::endl;
  }
  RunOptions run(opt);
  if (!run.read_replicates(opt, false)) return 1;
  const std::vector<double> age_grid = shared_age_grid();
  const int A = (int)age_grid.size(), B = run.B;
  const size_t P = pairs.size();
  const bool counts_only = opt.has("counts_only");
  const bool want_counts = counts_only || opt.has("counts_out");
  const DeviceWarmUp warm(opt);

  // ---- epochs per pair (coal.cpp:3501-3632): from the ages and --bins, or from the pair's coal= file (which also gives its
  // starting rates, coal.cpp:3638-3646): the launches are known before any file is read
  std::vector<std::vector<double>> epochs(P), init(P);
  std::vector<int> ep_null(P, 0);
  std::vector<double> age(P);
  for (size_t p = 0; p < P; p++) {
    age[p] = std::max(pairs[p].target_age, pairs[p].ref_age) / run.years_per_gen;
    const std::string* coal = pairs[p].coal.empty() ? nullptr : &pairs[p].coal;
    if (epochs_for(opt, coal, age[p], run.years_per_gen, epochs[p], init[p], ep_null[p]) <= 0) {
      std::cerr << "Error: pair " << p + 1 << ": " << colate_last_error() << std::endl;
      return 1;
    }
    if (coal && talk) {  // (as the single-pair CLI prints them, after the pair's number)
      std::cerr << "Pair " << p + 1 << ": ";
      for (double r : init[p]) std::cerr << r << " ";
      std::cerr << std::endl;
    }
  }
  // classes of pairs with the same number of epochs, in order of first appearance: one launch each
  const std::vector<std::vector<size_t>> classes = classes_by_epoch_count(epochs);
  // --ranks N: this rank's rows [lo, hi) of every class (row = position in the class * B + replicate) and the pairs they belong to
  std::vector<size_t> todo;
  std::vector<int> first_group(classes.size(), 0), group_count(classes.size(), 0);
  for (size_t c = 0; c < classes.size(); c++) {
    const int R = (int)(classes[c].size() * (size_t)B);
    int lo = 0, hi = R;
    if (g_rank.ranked) colate_shard_bounds(R, g_rank.nranks, g_rank.rank, &lo, &hi);
    if (counts_only && g_rank.ranked && g_rank.rank != 0) lo = hi = 0;
    if (hi > lo) {
      first_group[c] = lo / B;
      group_count[c] = (hi - 1) / B - lo / B + 1;
      for (int g = 0; g < group_count[c]; g++) todo.push_back(classes[c][(size_t)(first_group[c] + g)]);
    }
  }
  std::sort(todo.begin(), todo.end());

  std::vector<PairTables> tabs;
  if (!fill(todo, run.seed, A, tabs)) return 1;
  for (size_t p : todo) {
    if (talk) say_blocks(p, P, pairs[p], tabs[p].nb);
    if (tabs[p].nb < 1) {
      std::cerr << "Error: no genome blocks were read for pair " << p + 1 << "." << std::endl;
      return 1;
    }
  }
  // ---- bootstrap weights from each pair's own generator (coal.cpp:3350-3357)
  std::vector<std::vector<double>> weights(P);
  for (size_t p : todo) {
    weights[p].resize((size_t)B * tabs[p].nb);
    if (int rc = colate_bootstrap_weights(&tabs[p].rng, B, tabs[p].nb, weights[p].data())) return api_error(rc);
  }
  if (counts_only) {  // no device: the weighted sums and the F redistribution on the host (coal.cpp:3358-3451)
    for (size_t p : todo) {
      std::vector<double> csh((size_t)B * A), cns((size_t)B * A);
      PairTables& pt = tabs[p];
      if (int rc = colate_bootstrap_counts_from_weights(B, pt.nb, A, age_grid.data(), age[p], weights[p].data(), pt.sh.data(),
                                                        pt.ns.data(), pt.she.data(), pt.nse.data(), csh.data(), cns.data()))
        return api_error(rc);
      write_counts_file(pairs[p].output + ".counts", B, A, age_grid, csh.data(), cns.data());
    }
    return 0;
  }

  if (talk) std::cerr << "Maximising likelihood using EM.. " << std::endl;
  std::vector<int> dev_list;
  if (!bind_devices(opt, dev_list)) return 1;
  RankComm comm;
  if (g_rank.ranked && !comm.open(opt)) return 1;
  const double t_em0 = StageTimes::now();
  int status = 0;
  for (size_t c = 0; c < classes.size() && status == 0; c++) {
    const std::vector<size_t>& cls = classes[c];
    const int G = (int)cls.size(), E = (int)epochs[cls[0]].size();
    const size_t R = (size_t)G * B;
    const int g0 = first_group[c], gn = group_count[c];
    // this process's groups of the class, concatenated
    std::vector<int> nb(gn);
    std::vector<double> g_age(gn), g_w, g_sh, g_ns, g_she, g_nse, g_ep((size_t)gn * E), g_init((size_t)gn * E);
    for (int g = 0; g < gn; g++) {
      const size_t p = cls[(size_t)(g0 + g)];
      const PairTables& pt = tabs[p];
      nb[g] = pt.nb, g_age[g] = age[p];
      g_w.insert(g_w.end(), weights[p].begin(), weights[p].end());
      g_sh.insert(g_sh.end(), pt.sh.begin(), pt.sh.end());
      g_ns.insert(g_ns.end(), pt.ns.begin(), pt.ns.end());
      g_she.insert(g_she.end(), pt.she.begin(), pt.she.end());
      g_nse.insert(g_nse.end(), pt.nse.begin(), pt.nse.end());
      std::copy(epochs[p].begin(), epochs[p].end(), g_ep.begin() + (size_t)g * E);
      std::copy(init[p].begin(), init[p].end(), g_init.begin() + (size_t)g * E);
    }
    std::vector<double> rates(R * E), ll(R), csh, cns;
    std::vector<int> iters(R), flags(R);
    if (want_counts) csh.resize(R * A), cns.resize(R * A);
    int rc;
    if (g_rank.ranked) {
      rc = colate_bootstrap_em_batch_groups_allgather(comm.comm, G, B, g0, gn, E, A, age_grid.data(), nb.data(), g_age.data(), g_w.data(),
                                                      g_sh.data(), g_ns.data(), g_she.data(), g_nse.data(), g_ep.data(), g_init.data(),
                                                      COLATE_DEFAULT_MAX_ITER, COLATE_DEFAULT_MIN_ITER, COLATE_DEFAULT_REL_TOL,
                                                      COLATE_DEFAULT_RATE_FLOOR, rates.data(), iters.data(), ll.data(), flags.data());
    } else if (!dev_list.empty()) {
      // --devices N (one process, several GPUs): counts on the host, the rows sharded over GPUs 0..N-1
      csh.resize(R * A), cns.resize(R * A);
      rc = 0;
      for (int g = 0, wo = 0, bo = 0; g < G && !rc; wo += B * nb[g], bo += nb[g], g++)
        rc = colate_bootstrap_counts_from_weights(B, nb[g], A, age_grid.data(), g_age[g], g_w.data() + wo, g_sh.data() + (size_t)bo * A,
                                                  g_ns.data() + (size_t)bo * A, g_she.data() + (size_t)bo * A, g_nse.data() + (size_t)bo * A,
                                                  csh.data() + (size_t)g * B * A, cns.data() + (size_t)g * B * A);
      std::vector<double> r_ep(R * E), r_init(R * E);
      colate::expand_group_rows(g_ep.data(), (int)B, 0, 0, (long)R, E, r_ep.data());
      colate::expand_group_rows(g_init.data(), (int)B, 0, 0, (long)R, E, r_init.data());
      if (!rc)
        rc = colate_em_batch_rows_sharded((int)dev_list.size(), dev_list.data(), (int)R, E, A, age_grid.data(), csh.data(), cns.data(),
                                          r_ep.data(), r_init.data(), COLATE_DEFAULT_MAX_ITER, COLATE_DEFAULT_MIN_ITER,
                                          COLATE_DEFAULT_REL_TOL, COLATE_DEFAULT_RATE_FLOOR, rates.data(), iters.data(), ll.data(),
                                          flags.data());
    } else {
      rc = colate_bootstrap_em_batch_groups(G, B, E, A, age_grid.data(), nb.data(), g_age.data(), g_w.data(), g_sh.data(), g_ns.data(),
                                            g_she.data(), g_nse.data(), g_ep.data(), g_init.data(), COLATE_DEFAULT_MAX_ITER,
                                            COLATE_DEFAULT_MIN_ITER, COLATE_DEFAULT_REL_TOL, COLATE_DEFAULT_RATE_FLOOR, rates.data(),
                                            iters.data(), ll.data(), flags.data(), want_counts ? csh.data() : nullptr,
                                            want_counts ? cns.data() : nullptr);
    }
    if (rc) {
      status = api_error(rc);
      break;
    }
    if (!talk) continue;
    for (int g = 0; g < G; g++) {
      const size_t p = cls[(size_t)g];
      report_bootstraps((int)p + 1, B, E, iters.data() + (size_t)g * B, flags.data() + (size_t)g * B, true);
      if (want_counts && !csh.empty())
        write_counts_file(pairs[p].output + ".counts", B, A, age_grid, csh.data() + (size_t)g * B * A, cns.data() + (size_t)g * B * A);
      if (!write_coal(pairs[p].output, B, E, epochs[p].data(), rates.data() + (size_t)g * B * E, age[p] > 0.0, ep_null[p])) {
        status = 1;
        break;
      }
    }
  }
  g_times.bootstrap_em = StageTimes::now() - t_em0;
  if (g_times.on)
    std::cerr << "Timing: inputs " << g_times.parse_mut << " s, pairs' table fill " << g_times.table_fill << " s, bootstrap_em "
              << g_times.bootstrap_em << " s" << std::endl;
  if (status || !talk) return status;
  print_usage_footer();
  return 0;
}

int run_mut_pairs(const Options& opt) {
  if (!opt.has("mut")) {
    std::cerr << "Error: --pairs needs --mut (and optionally --chr, --bins, --num_bootstraps, --seed)." << std::endl;
    return 1;
  }
  if (refuse_per_line_options(opt)) return 1;
  std::vector<std::string> chr_names, mut_files;
  chromosome_files(opt, chr_names, mut_files);  // (once: the list's mask prefixes expand with these names, and the fill reads these files)
  std::vector<PairSpec> pairs;
  if (!read_pair_list(opt.get("pairs"), opt, chr_names, pairs)) return 1;
  if (!pairs_have_epochs(opt, pairs)) return 1;
  return run_pair_list(opt, pairs, [&](const std::vector<size_t>& todo, int seed, int A, std::vector<PairTables>& tabs) {
    return fill_pairs(opt, chr_names, mut_files, pairs, todo, seed, A, tabs);
  });
}

// `Colate --mode mut --samples LIST`: every (target line, reference line) of the list, each pair's files byte for byte what
// `--pairs` writes for the expanded list.  The tables come from fill_sample_pairs (fill_samples.cpp): walked and filled on the
// device where there is one, else through fill_pairs.
int run_mut_samples(const Options& opt) {
  if (refuse_options(opt, {"pairs", "target_tmp", "reference_tmp", "target_mask", "reference_mask", "target_age", "reference_age", "ranks"},
                     "--mode mut --samples"))
    return 1;
  if (!opt.has("mut") || !opt.has("output") || (!opt.has("bins") && !opt.has("coal"))) {
    std::cerr << "Error: --samples needs --mut, -o PREFIX and --bins x,y,stepsize or --coal FILE (optional: --chr, --num_bootstraps, --seed, "
                 "--years_per_gen, --counts_out, --counts_only, --device, --devices)."
              << std::endl;
    return 1;
  }
  std::vector<std::string> chr_names, mut_files;
  chromosome_files(opt, chr_names, mut_files);
  std::vector<SampleLine> samples;
  if (!read_sample_list(opt.get("samples"), opt, chr_names, true, samples)) return 1;
  std::vector<PairSpec> pairs;
  if (!sample_pairs(samples, opt.get("output"), opt.get("samples"), pairs)) return 1;
  if (!opt.has("bins"))
    for (PairSpec& ps : pairs) ps.coal = opt.get("coal");
  return run_pair_list(opt, pairs, [&](const std::vector<size_t>& todo, int seed, int A, std::vector<PairTables>& tabs) {
    return fill_sample_pairs(opt, chr_names, mut_files, pairs, todo, seed, A, tabs);
  });
}

// `--mode mut`: the list forms, the launcher of `--ranks`, or the single pair
static int run_mut_mode(const Options& opt) {
  if (opt.has("help")) {
    print_help();
    std::cout << "Calculate coalescence rates for sample." << std::endl;
    return 0;
  }
  if (opt.has("samples")) return run_mut_samples(opt);  // (refuses --ranks by name)
  if (opt.has("ranks")) {
    const int nranks = opt.get_int("ranks");
    if (nranks < 1 || nranks > 64) {
      std::cerr << "Error: --ranks must be between 1 and 64." << std::endl;
      return 1;
    }
    if (opt.has("mut") && (opt.has("output") || opt.has("pairs"))) return run_ranked(opt, nranks);  // (also for N = 1: same code path)
  }
  if (opt.has("pairs")) return run_mut_pairs(opt);
  return run_mut(opt);
}

}  // namespace colate_drv

using namespace colate_drv;

extern "C" int colate_mut_main(int argc, char** argv) {
  Options opt;
  std::string err;
  if (!parse_options(argc, argv, opt, err)) {
    std::cerr << err << std::endl;
    return 1;
  }
  if (!opt.has("mode")) {  // Colate.cpp:104-112
    std::cout << "Not enough arguments supplied." << std::endl;
    print_help();
    return 0;
  }
  const std::string& mode = opt.get("mode");
  for (const char* o : {"age_profile", "profile_only", "jackknife", "block_bases", "expected"})
    if (opt.has(o) && mode != "count_topo") {
      std::cerr << "Error: --" << o << " is an option of --mode count_topo --samples." << std::endl;
      return 1;
    }
  static const struct {
    const char* mode;
    int (*run)(const Options&);
  } kModes[] = {{"mut", run_mut_mode},         {"mut_interval", run_mut_interval}, {"compare_tmp", run_compare_tmp},
                {"count_topo", run_count_topo}, {"make_tmp", run_make_tmp},         {"CondCoalRates", run_condcoal}};
  for (const auto& m : kModes) {
    if (mode != m.mode) continue;
    try {
      return m.run(opt);
    } catch (const std::exception& e) {  // (an option whose text is no number: std::stoi / std::stof)
      std::cerr << "Error: " << e.what() << std::endl;
      return 1;
    }
  }
  std::cout << "####### error #######" << std::endl;
  std::cout << "colate_amd implements --mode mut, --mode mut_interval, --mode compare_tmp, --mode count_topo, --mode make_tmp --target_table and --mode "
               "CondCoalRates (preprocess_mut, make_tmp from BCF/BAM, calc_depth, print_tmp stay with the reference build)."
            << std::endl;
  return 1;
}
