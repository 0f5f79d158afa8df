// colate_amd/csrc/topo_driver.cpp -- `Colate --mode count_topo` (count_topo.h: the contract, include/coal/coal.cpp:4523-4781): the
// SNPs at which the conditioning sample carries the derived allele and an allele sampled from the target differs from one
// sampled from the reference, with the sign of the difference.
//   * `-i C --target_tmp T --reference_tmp R --mut P -o OUT [--chr FILE] [--seed S]`: the reference's single run, OUT byte for
//     byte its file for the same --seed.  The cursor walk on the host; no device is opened.  COLATE_DEVICE_TOPO=1 sends the
//     triple through the indexed path below as a list of one.
//   * `--samples LIST --mut P -o PREFIX [--chr FILE] [--seed S] [--device D]`: every (cond line, target line, reference line) of
//     three different lines of the list, cond outermost, then target, then reference; PREFIX_<cond>_<target>_<reference>.txt is
//     the single run's file with the same --seed, PREFIX.triples.txt holds one line `cond target reference plus minus draws` per
//     triple.  The rows, one walk index and one cond index per sample are staged once and colate_topo_samples draws every triple
//     on the device; its host twin without a device or with COLATE_DEVICE_TOPO=0; the cursor walk per triple where a sample
//     cannot be indexed.  All three give the same bytes.
//     `--age_profile x,y,s [--years_per_gen Y]`: besides, PREFIX.profile.txt with one line `cond target reference epoch plus minus
//     qualifying` per (triple, epoch) -- the printed rows of either sign and the rows that drew, binned by the mid of their ages
//     (count_topo.h: age_epoch) into the epochs of `--mode mut --bins x,y,s` -- through colate_topo_profile, a second pass over the
//     staged inputs.  `--profile_only`: no per-triple file; PREFIX.triples.txt from the profile's sums, the same bytes; only the
//     profile call runs, and no plane, bit or line is formed.
//     `--jackknife [--block_bases N]` (with --age_profile; N >= 1, default 30000000): besides, PREFIX.jackknife.txt with one line
//     `cond target reference epoch plus minus blocks D D_jack se Z` per (triple, epoch) and, last of a triple, for epoch `all` --
//     the delete-one block jackknife of count_topo.h over the genome blocks of this mode, which are a function of the searched rows
//     alone.  The counts per (triple, block, epoch) come from colate_topo_profile_blocks in place of the profile call (its host twin;
//     on the cursor path the walk's sinks bin by block); PREFIX.profile.txt and PREFIX.triples.txt are formed from their sums over
//     the blocks, the same bytes as without the option.
//     `--expected [--jackknife [--block_bases N]]` (with --age_profile): nothing sampled is written; PREFIX.expected.txt holds one line
//     `cond target reference epoch plus minus qualifying` per (triple, epoch) with plus and minus the EXPECTED counts given the read
//     counts -- the sums of pT (1 - pR) and (1 - pT) pR over the qualifying rows, formed in units of 2^-30 by
//     colate_topo_expected_blocks (its host twin; the cursor walk's `drew` sink) and printed %.6f --, and with --jackknife
//     PREFIX.expected.jackknife.txt the columns of PREFIX.jackknife.txt from those integers as they are.  No stream of uniforms is
//     formed; --seed is accepted and has no effect.
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <random>
#include <string>
#include <vector>

#include "cli_lists.h"
#include "cli_modes.h"
#include "colate_amd.h"
#include "count_topo.h"
#include "walk_inputs.h"

namespace colate_drv {

namespace {

// One triple's file: `name pos age_begin age_end sign value`, the ages floats and the value a double in the stream's default
// format (coal.cpp:4746, 4748).
bool write_lines(const std::string& path, const std::vector<std::string>& names, const std::vector<TopoLine>& lines) {
  std::ofstream os(path);
  for (const TopoLine& l : lines) {
    os << names[(size_t)l.chr] << " " << l.pos << " " << l.age_begin << " " << l.age_end << " ";
    if (l.sign > 0) os << 1 << " " << ((double)l.DAF) / l.N << "\n";
    else os << -1 << " " << -((double)l.DAF) / l.N << "\n";
  }
  return close_checked(os, path);
}

double g_triple_stage_s = 0;  // the seconds of the triple stage alone, whichever forms ran (COLATE_TIMING)
double g_kernel_s = 0;        // ... and of its kernels on the device

// The inputs of `triples` (PairSpec with its cond file) as every form of the triple stage takes them: loaded once, the form
// decided, and -- for the two indexed forms -- the run's stream (stage_triples with stream = false: none, `--expected` draws
// nothing) and the view.
struct Staged {
  WalkInputs in;
  Path path = Path::cursors;
  unsigned seed = 0;
  std::vector<double> u;
  std::vector<colate_topo::Triple> ids;
  colate_topo::View v;
  const char* where() const { return path == Path::device ? "device" : "host"; }
};

// False after an error message; nothing has been written then.
bool stage_triples(const Options& opt, const std::vector<std::string>& names, const std::vector<std::string>& mut_files,
                   const std::vector<PairSpec>& triples, Path want, unsigned seed, Staged& st, bool stream = true) {
  WalkInputs& in = st.in;
  std::vector<const std::string*> files;
  for (const PairSpec& ps : triples) files.insert(files.end(), {&ps.cond, &ps.target, &ps.reference});  // coal.cpp:4588-4603
  if (!check_readable(files, "Failed to open")) return false;
  if (!load_walk_inputs(names, mut_files, triples, in, RowSet::count_topo)) return false;
  if (!in.files_ok) {
    std::cerr << "Error: a .colate.in file could not be read." << std::endl;
    return false;
  }
  const size_t P = triples.size();
  if (want != Path::cursors && !in.indexed) {
    std::cerr << "triples drawn on the host through the record cursors (a sample has no walk index: counts beyond 16 bits, an empty chromosome "
                 "name, or rows that descend)"
              << std::endl;
    want = Path::cursors;
  }
  st.path = want, st.seed = seed;
  if (want == Path::cursors) return true;
  const int C = (int)names.size();
  const long long n_rows = in.row_off.back();
  // the run's stream: a row draws two uniforms at most, and every triple starts from the seed
  if (stream) {
    st.u.resize((size_t)(2 * n_rows));
    std::mt19937 rng(seed);
    std::uniform_real_distribution<double> dist_unif(0, 1);
    for (double& x : st.u) x = dist_unif(rng);
  }
  st.ids.resize(P);
  for (size_t p = 0; p < P; p++) st.ids[p] = colate_topo::Triple{in.cond_ids[p], in.pairs[p].target, in.pairs[p].reference};
  colate_topo::View& v = st.v;
  v.C = C, v.row_off = in.row_off.data(), v.rows = in.row_ptrs.data(), v.S = in.S, v.idx = in.idx_ptrs.data(), v.cidx = in.cidx_ptrs.data();
  v.P = (int)P, v.triples = st.ids.data(), v.n_uniforms = (long long)st.u.size(), v.uniforms = st.u.data();
  return want != Path::device || bind_device(opt);
}

// Draws every staged triple: the lines each prints and its qualifying rows.  profile: on the cursor path the same walk fills it.
bool draw_triples(const Staged& st, const std::vector<std::string>& names, const std::vector<PairSpec>& triples,
                  std::vector<std::vector<TopoLine>>& lines, std::vector<long long>& draws, TopoProfile* profile = nullptr) {
  const WalkInputs& in = st.in;
  const size_t P = triples.size();
  const double t_stage = StageTimes::now();
  if (st.path == Path::cursors) {
    const bool ok = topo_cursor_triples(in, names, triples, st.seed, lines, draws, profile);
    g_triple_stage_s += StageTimes::now() - t_stage;
    return ok;
  }
  const int C = (int)names.size();
  const colate_topo::View& v = st.v;
  const std::vector<colate_topo::Triple>& ids = st.ids;
  std::vector<long long> word_off((size_t)C + 1);
  const long long words = colate_iw::mask_words(C, v.row_off, word_off.data());
  std::vector<unsigned long long> plus(P * (size_t)words), minus(P * (size_t)words);
  draws.assign(P, 0);
  const long long cap = (long long)P * words;
  if (int rc = st.path == Path::device ? colate_topo::topo_view_device(v, cap, word_off.data(), plus.data(), minus.data(), draws.data())
                                       : colate_topo::topo_view_host(v, cap, word_off.data(), plus.data(), minus.data(), draws.data()))
    return api_error(rc), false;
  g_triple_stage_s += StageTimes::now() - t_stage;
  g_kernel_s += colate_topo_samples_kernel_seconds();
  // set bits into lines; the value is that of the conditioning record, which the cond index holds
  lines.assign(P, std::vector<TopoLine>());
  for (size_t p = 0; p < P; p++)
    for (int c = 0; c < C; c++) {
      const colate_walk_row* const rows = in.row_ptrs[(size_t)c];
      const colate_walk_idx* const ci = in.cidx_ptrs[(size_t)ids[p].cond * C + c];
      for (long long k = word_off[(size_t)c]; k < word_off[(size_t)c + 1]; k++) {
        const unsigned long long a = plus[p * (size_t)words + (size_t)k], b = minus[p * (size_t)words + (size_t)k];
        for (unsigned long long q = a | b; q; q &= q - 1) {
          const int bit = __builtin_ctzll(q);
          const long long i = (k - word_off[(size_t)c]) * 64 + bit;
          lines[p].push_back(TopoLine{c, rows[i].pos, rows[i].age_begin, rows[i].age_end, (a >> bit) & 1 ? 1 : -1, (int)ci[i].DAF,
                                      (int)ci[i].DAF + (int)ci[i].AAF});
        }
      }
    }
  std::cerr << in.S << " samples staged, " << P << " triples drawn on the " << st.where() << std::endl;
  return true;
}

// profile.counts[P][E][3], zeros before, from the sums of profile.blocks[P][nb][E][3] over the blocks
void sum_blocks(TopoProfile& profile, size_t P, int nb) {
  const size_t per_block = (size_t)profile.E * 3;
  for (size_t p = 0; p < P; p++)
    for (size_t b = 0; b < (size_t)nb; b++)
      for (size_t k = 0; k < per_block; k++) profile.counts[p * per_block + k] += profile.blocks[(p * (size_t)nb + b) * per_block + k];
}

// The age profile of every staged triple (count_topo.h: age_epoch): profile.counts[P][E][3] and the qualifying rows.  No plane and
// no line is formed on the indexed forms.  With profile.nbpb > 0 (`--jackknife`) profile.blocks[P][nb][E][3] is formed, per genome
// block, and profile.counts from its sums over the blocks.
bool profile_triples(const Staged& st, const std::vector<std::string>& names, const std::vector<PairSpec>& triples, TopoProfile& profile,
                     std::vector<long long>& draws) {
  const size_t P = triples.size();
  const double t_stage = StageTimes::now();
  if (st.path == Path::cursors) {
    std::vector<std::vector<TopoLine>> lines;
    const bool ok = topo_cursor_triples(st.in, names, triples, st.seed, lines, draws, &profile);
    g_triple_stage_s += StageTimes::now() - t_stage;
    return ok;
  }
  profile.counts.assign(P * (size_t)profile.E * 3, 0);
  draws.assign(P, 0);
  if (profile.nbpb > 0) {
    const int nb = profile.blk_off[st.v.C];
    const size_t per_block = (size_t)profile.E * 3;
    profile.blocks.assign(P * (size_t)nb * per_block, 0);
    if (int rc = st.path == Path::device
                     ? colate_topo::topo_profile_blocks_device(st.v, profile.E, profile.epochs, profile.nbpb, nb, profile.blocks.data(), draws.data())
                     : colate_topo::topo_profile_blocks_host(st.v, profile.E, profile.epochs, profile.nbpb, nb, profile.blocks.data(), draws.data()))
      return api_error(rc), false;
    sum_blocks(profile, P, nb);
    g_triple_stage_s += StageTimes::now() - t_stage;
    g_kernel_s += colate_topo_profile_blocks_kernel_seconds();
    std::cerr << st.in.S << " samples staged, " << P << " triples profiled in " << nb << " blocks on the " << st.where() << std::endl;
    return true;
  }
  if (int rc = st.path == Path::device ? colate_topo::topo_profile_device(st.v, profile.E, profile.epochs, profile.counts.data(), draws.data())
                                       : colate_topo::topo_profile_host(st.v, profile.E, profile.epochs, profile.counts.data(), draws.data()))
    return api_error(rc), false;
  g_triple_stage_s += StageTimes::now() - t_stage;
  g_kernel_s += colate_topo_profile_kernel_seconds();
  std::cerr << st.in.S << " samples staged, " << P << " triples profiled on the " << st.where() << std::endl;
  return true;
}

// `--expected`: the expected counts of every staged triple per genome block and epoch (count_topo.h: the expected counts), in units
// of 2^-30: profile.blocks[P][nb][E][3] and profile.counts, their sums over the blocks.  No stream, no draw.
bool expected_triples(const Staged& st, const std::vector<std::string>& names, const std::vector<PairSpec>& triples, TopoProfile& profile) {
  const size_t P = triples.size();
  const double t_stage = StageTimes::now();
  if (st.path == Path::cursors) {
    const bool ok = topo_cursor_expected(st.in, names, triples, profile);
    g_triple_stage_s += StageTimes::now() - t_stage;
    return ok;
  }
  const int nb = profile.blk_off[st.v.C];
  const size_t per_block = (size_t)profile.E * 3;
  profile.counts.assign(P * per_block, 0), profile.blocks.assign(P * (size_t)nb * per_block, 0);
  if (int rc = st.path == Path::device
                   ? colate_topo::topo_expected_blocks_device(st.v, profile.E, profile.epochs, profile.nbpb, nb, profile.blocks.data())
                   : colate_topo::topo_expected_blocks_host(st.v, profile.E, profile.epochs, profile.nbpb, nb, profile.blocks.data()))
    return api_error(rc), false;
  sum_blocks(profile, P, nb);
  g_triple_stage_s += StageTimes::now() - t_stage;
  g_kernel_s += colate_topo_expected_blocks_kernel_seconds();
  std::cerr << st.in.S << " samples staged, " << P << " triples expected in " << nb << " blocks on the " << st.where() << std::endl;
  return true;
}

// %.6g, NA for "not available"
std::string stat_text(double x) {
  char text[40];
  std::snprintf(text, sizeof(text), "%.6g", x);
  return std::isnan(x) ? std::string("NA") : std::string(text);
}

// a fixed-point sum as the expected files print it: %.6f of (double)sum * 2^-30
std::string fixed_text(long long sum) {
  char text[48];
  std::snprintf(text, sizeof(text), "%.6f", (double)sum * 0x1p-30);
  return text;
}

// a sampled count as the profile files print it
std::string integer_text(long long n) { return std::to_string(n); }

// PREFIX.profile.txt and PREFIX.expected.txt: `cond target reference epoch plus minus qualifying` per (triple, epoch), every epoch of
// every triple, the epoch as a .coal prints it; print_count: plus and minus as the file prints them (integer_text, fixed_text).
bool write_epoch_table(const std::string& path, const std::vector<std::string>& triple_names, const std::vector<double>& epochs,
                       const TopoProfile& profile, std::string (*print_count)(long long)) {
  std::ofstream os(path);
  for (size_t p = 0; p < triple_names.size(); p++)
    for (int e = 0; e < profile.E; e++) {
      const long long* const x = &profile.counts[(p * (size_t)profile.E + (size_t)e) * 3];
      os << triple_names[p] << " " << epochs[(size_t)e] << " " << print_count(x[0]) << " " << print_count(x[1]) << " " << x[2] << "\n";
    }
  return close_checked(os, path);
}

// PREFIX.jackknife.txt and PREFIX.expected.jackknife.txt: `cond target reference epoch plus minus blocks D D_jack se Z` per (triple,
// epoch) and, last of a triple, for epoch `all`; the statistics from profile.blocks as they are -- sampled counts, or the fixed-point
// integers of the expected counts.
bool write_jackknife(const std::string& path, const std::vector<std::string>& triple_names, const std::vector<double>& epochs,
                     const TopoProfile& profile, int nb, std::string (*print_count)(long long)) {
  const int E = profile.E;
  std::ofstream jk(path);
  std::vector<double> stats(((size_t)E + 1) * 4);
  std::vector<int> used((size_t)E + 1);
  for (size_t p = 0; p < triple_names.size(); p++) {
    colate_topo::jackknife(nb, E, &profile.blocks[p * (size_t)nb * (size_t)E * 3], stats.data(), used.data());
    long long plus = 0, minus = 0;
    for (int e = 0; e <= E; e++) {
      jk << triple_names[p] << " ";
      if (e < E) {
        const long long* const x = &profile.counts[(p * (size_t)E + (size_t)e) * 3];
        plus += x[0], minus += x[1];
        jk << epochs[(size_t)e] << " " << print_count(x[0]) << " " << print_count(x[1]);
      } else {
        jk << "all " << print_count(plus) << " " << print_count(minus);
      }
      const double* const o = &stats[(size_t)e * 4];
      jk << " " << used[(size_t)e] << " " << stat_text(o[0]) << " " << stat_text(o[1]) << " " << stat_text(o[2]) << " " << stat_text(o[3]) << "\n";
    }
  }
  return close_checked(jk, path);
}

// the line of COLATE_TIMING; t0: the start of the inputs, t1: the start of the files
void print_timing(double t0, double t1, const WalkInputs& in, size_t triples) {
  if (!g_times.on) return;
  std::cerr << "Timing: count_topo samples: inputs " << t1 - t0 - g_triple_stage_s << " s, triple stage " << g_triple_stage_s << " s (device kernels "
            << g_kernel_s << " s), files " << StageTimes::now() - t1 << " s; " << (in.row_off.empty() ? 0LL : in.row_off.back()) << " rows, " << in.S
            << " samples, " << triples << " triples" << std::endl;
}

int run_topo_samples(const Options& opt) {
  if (refuse_options(opt, {"input", "pairs", "target_tmp", "reference_tmp", "target_mask", "reference_mask", "target_age", "reference_age", "bins",
                           "coal", "num_bootstraps", "ranks", "devices"},
                     "--mode count_topo --samples"))
    return 1;
  if (!opt.has("mut") || !opt.has("output")) {
    std::cerr << "Error: --samples needs --mut and -o PREFIX (optional: --chr, --seed, --device, --age_profile, --years_per_gen, --profile_only)."
              << std::endl;
    return 1;
  }
  // `--age_profile x,y,s`: the epochs a .coal of `--mode mut --bins x,y,s` prints, in generations
  const bool profiled = opt.has("age_profile"), profile_only = opt.has("profile_only");
  if (profile_only && !profiled) {
    std::cerr << "Error: --profile_only needs --age_profile x,y,stepsize." << std::endl;
    return 1;
  }
  // `--expected`: the expected counts in place of everything sampled
  const bool expected = opt.has("expected");
  if (expected && profile_only) {
    std::cerr << "Error: --profile_only does not go with --expected, which writes no sampled file." << std::endl;
    return 1;
  }
  if (expected && !profiled) {
    std::cerr << "Error: --expected needs --age_profile x,y,stepsize." << std::endl;
    return 1;
  }
  // `--jackknife [--block_bases N]`: the genome blocks of count_topo.h, N bases each
  const bool jackknifed = opt.has("jackknife");
  if (jackknifed && !profiled) {
    std::cerr << "Error: --jackknife needs --age_profile x,y,stepsize." << std::endl;
    return 1;
  }
  if (opt.has("block_bases") && !jackknifed) {
    std::cerr << "Error: --block_bases needs --jackknife." << std::endl;
    return 1;
  }
  int block_bases = kIntervalBasesPerBlock;
  if (opt.has("block_bases")) {
    const std::string& text = opt.get("block_bases");
    char* end = nullptr;
    const long long n = std::strtoll(text.c_str(), &end, 10);
    if (text.empty() || *end != '\0' || n < 1 || n > INT_MAX) {
      std::cerr << "Error: --block_bases takes an integer of at least 1 (given: " << text << ")." << std::endl;
      return 1;
    }
    block_bases = (int)n;
  }
  std::vector<double> epochs, boundaries;
  TopoProfile profile;
  if (profiled) {
    const double years_per_gen = RunOptions(opt).years_per_gen;
    epochs.resize(colate_topo::kMaxProfileEpochs);
    const int E = colate_epochs_from_bins(opt.get("age_profile").c_str(), 0.0, years_per_gen, epochs.data(), (int)epochs.size(), nullptr);
    if (E < 0) return api_error(E);
    epochs.resize((size_t)E);
    // With age 0 the reference's epochs start 0, 0: epoch 0 is [0, 0) and holds the rows of a negative mid only.  age_epoch reads
    // epochs[1 .. E - 1] alone, so every form bins over the same boundaries with epochs[0] moved below epochs[1], which ascend
    // strictly as the call demands; the file prints the reference's.
    boundaries = epochs;
    if (E >= 2 && boundaries[0] >= boundaries[1]) boundaries[0] = boundaries[1] - 1.0;
    if (int rc = colate_topo::check_epochs(E, boundaries.data())) return api_error(rc);
    profile.E = E, profile.epochs = boundaries.data();
  }
  std::vector<std::string> names, mut_files;
  chromosome_files(opt, names, mut_files);
  std::vector<SampleLine> samples;
  if (!read_sample_list(opt.get("samples"), opt, names, false, samples, true)) return 1;
  for (const SampleLine& sl : samples)
    if (!sl.masks.empty()) {
      std::cerr << "Error: " << opt.get("samples") << ", line " << sl.line << ": mask= is not supported by --mode count_topo" << std::endl;
      return 1;
    }
  std::vector<PairSpec> triples;
  std::vector<std::string> triple_names;
  for (const SampleLine& c : samples)
    for (const SampleLine& t : samples)
      for (const SampleLine& r : samples) {
        if (!c.cond || !t.target || !r.reference || &c == &t || &c == &r || &t == &r) continue;
        PairSpec ps;
        ps.cond = c.file, ps.target = t.file, ps.reference = r.file, ps.line = c.line;
        ps.output = opt.get("output") + "_" + c.name + "_" + t.name + "_" + r.name + ".txt";
        triples.push_back(ps);
        triple_names.push_back(c.name + " " + t.name + " " + r.name);
      }
  if (triples.empty()) {
    std::cerr << "Error: " << opt.get("samples") << ": no triple of a cond, a target and a reference on three different lines." << std::endl;
    return 1;
  }
  const unsigned seed = (unsigned)run_seed(opt);
  std::cerr << "---------------------------------------------------------" << std::endl;
  std::cerr << "Counting topologies for " << triples.size() << " triples.." << std::endl;
  std::string why;
  const Path want = choose_path("COLATE_DEVICE_TOPO", true, why);
  if (want != Path::device) std::cerr << "triples drawn on the host (" << why << ")" << std::endl;
  const double t0 = StageTimes::now();
  Staged st;
  std::vector<std::vector<TopoLine>> lines;
  std::vector<long long> draws;
  if (!stage_triples(opt, names, mut_files, triples, want, seed, st, !expected)) return 1;
  const WalkInputs& in = st.in;
  const bool one_walk = st.path == Path::cursors;  // (the cursor walk fills lines and profile at once)
  std::vector<int> blk_off;
  if (jackknifed || expected) {  // the blocks are those of the searched rows, whichever form walks them
    blk_off.resize(names.size() + 1);
    if (int rc = one_walk ? topo_cursor_blocks(in, block_bases, blk_off)
                          : colate_topo::topo_blocks(st.v.C, st.v.row_off, st.v.rows, block_bases, blk_off.data()))
      return api_error(rc);
    profile.nbpb = block_bases, profile.blk_off = blk_off.data();
  }
  if (expected) {  // (the file does not depend on the blocks: without --jackknife they are the default's)
    if (!expected_triples(st, names, triples, profile)) return 1;
    const double t1 = StageTimes::now();
    if (!write_epoch_table(opt.get("output") + ".expected.txt", triple_names, epochs, profile, fixed_text)) return 1;
    if (jackknifed && !write_jackknife(opt.get("output") + ".expected.jackknife.txt", triple_names, epochs, profile, blk_off.back(), fixed_text)) return 1;
    print_timing(t0, t1, in, triples.size());
    print_usage_footer();
    return 0;
  }
  if (!profile_only && !draw_triples(st, names, triples, lines, draws, profiled && one_walk ? &profile : nullptr)) return 1;
  if (profiled && (profile_only || !one_walk) && !profile_triples(st, names, triples, profile, draws)) return 1;
  const double t1 = StageTimes::now();
  std::ofstream os(opt.get("output") + ".triples.txt");
  for (size_t p = 0; p < triples.size(); p++) {
    long long plus = 0, minus = 0;
    if (profile_only) {  // the profile's sums: the same totals
      for (int e = 0; e < profile.E; e++)
        plus += profile.counts[(p * (size_t)profile.E + (size_t)e) * 3], minus += profile.counts[(p * (size_t)profile.E + (size_t)e) * 3 + 1];
    } else {
      if (!write_lines(triples[p].output, names, lines[p])) return 1;
      for (const TopoLine& l : lines[p]) (l.sign > 0 ? plus : minus)++;
    }
    os << triple_names[p] << " " << plus << " " << minus << " " << draws[p] << "\n";
  }
  if (!close_checked(os, opt.get("output") + ".triples.txt")) return 1;
  if (profiled && !write_epoch_table(opt.get("output") + ".profile.txt", triple_names, epochs, profile, integer_text)) return 1;
  if (jackknifed && !write_jackknife(opt.get("output") + ".jackknife.txt", triple_names, epochs, profile, blk_off.back(), integer_text)) return 1;
  print_timing(t0, t1, in, triples.size());
  print_usage_footer();
  return 0;
}

}  // namespace

int run_count_topo(const Options& opt) {
  if (opt.has("samples")) return run_topo_samples(opt);
  for (const char* o : {"age_profile", "profile_only", "jackknife", "block_bases", "expected"})
    if (opt.has(o)) {
      std::cerr << "Error: --" << o << " needs --mode count_topo --samples: the single run of one triple writes its SNP lines only." << std::endl;
      return 1;
    }
  const bool missing = !opt.has("target_tmp") || !opt.has("reference_tmp") || !opt.has("input") || !opt.has("mut") || !opt.has("output");
  if (missing || opt.has("help")) {  // coal.cpp:4528-4538
    if (missing) {
      std::cout << "Not enough arguments supplied." << std::endl;
      std::cout << "Needed: target_tmp, reference_tmp, input, mut, output. Optional: chr." << std::endl;
    }
    print_help();
    std::cout << "Compare tmp." << std::endl;
    return 0;
  }
  std::cerr << "---------------------------------------------------------" << std::endl;
  std::cerr << "Calculating Colate tmp input file for " << opt.get("target_tmp") << ".." << std::endl;
  const unsigned seed = (unsigned)run_seed(opt);
  std::vector<std::string> names, mut_files;
  chromosome_files(opt, names, mut_files);
  PairSpec ps;
  ps.cond = opt.get("input"), ps.target = opt.get("target_tmp"), ps.reference = opt.get("reference_tmp"), ps.output = opt.get("output");
  std::string why;
  const Path want = choose_path("COLATE_DEVICE_TOPO", false, why);
  const std::vector<PairSpec> one(1, ps);
  Staged st;
  std::vector<std::vector<TopoLine>> lines;
  std::vector<long long> draws;
  if (!stage_triples(opt, names, mut_files, one, want, seed, st) || !draw_triples(st, names, one, lines, draws)) return 1;
  if (!write_lines(ps.output, names, lines[0])) return 1;
  print_usage_footer();
  return 0;
}

}  // namespace colate_drv
