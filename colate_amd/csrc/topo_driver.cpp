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
#include <unistd.h>

#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <ctime>
#include <fstream>
#include <iostream>
#include <random>
#include <string>
#include <vector>

#include "colate_amd.h"
#include "count_topo.h"
#include "mut_feeder.h"

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
  os.close();
  if (!os) {
    std::cerr << "Error: cannot write " << path << std::endl;
    return false;
  }
  return true;
}

enum class Path { cursors, host_twin, device };
double g_triple_stage_s = 0;  // the seconds of the triple stage alone, whichever form ran (COLATE_TIMING)

unsigned run_seed(const Options& opt) {  // coal.cpp:4545-4549
  int seed = (int)(std::time(nullptr) + getpid());
  if (opt.has("seed")) seed = std::stoi(opt.get("seed"));
  return (unsigned)seed;
}

// Loads the inputs of `triples` (PairSpec with its cond file) and draws every triple: the lines each prints and its qualifying
// rows.  False after an error message; nothing has been written then.
bool draw_triples(const Options& opt, const std::vector<std::string>& names, const std::vector<std::string>& mut_files,
                  const std::vector<PairSpec>& triples, Path want, unsigned seed, WalkInputs& in, std::vector<std::vector<TopoLine>>& lines,
                  std::vector<long long>& draws) {
  for (const PairSpec& ps : triples)
    for (const std::string* f : {&ps.cond, &ps.target, &ps.reference}) {  // coal.cpp:4588-4603
      FILE* fp = std::fopen(f->c_str(), "rb");
      if (!fp) {
        std::cerr << "Error: Failed to open " << *f << std::endl;
        return false;
      }
      std::fclose(fp);
    }
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
  const double t_stage = StageTimes::now();
  if (want == Path::cursors) {
    const bool ok = topo_cursor_triples(in, names, triples, seed, lines, draws);
    g_triple_stage_s = StageTimes::now() - t_stage;
    return ok;
  }
  const int C = (int)names.size();
  const long long n_rows = in.row_off.back();
  // the run's stream: a row draws two uniforms at most, and every triple starts from the seed
  std::vector<double> u((size_t)(2 * n_rows));
  {
    std::mt19937 rng(seed);
    std::uniform_real_distribution<double> dist_unif(0, 1);
    for (double& x : u) x = dist_unif(rng);
  }
  std::vector<colate_topo::Triple> ids(P);
  for (size_t p = 0; p < P; p++) ids[p] = colate_topo::Triple{in.cond_ids[p], in.pairs[p].target, in.pairs[p].reference};
  colate_topo::View v;
  v.C = C, v.row_off = in.row_off.data(), v.rows = in.row_ptrs.data(), v.S = in.S, v.idx = in.idx_ptrs.data(), v.cidx = in.cidx_ptrs.data();
  v.P = (int)P, v.triples = ids.data(), v.n_uniforms = (long long)u.size(), v.uniforms = u.data();
  std::vector<long long> word_off((size_t)C + 1);
  const long long words = colate_iw::mask_words(C, v.row_off, word_off.data());
  std::vector<unsigned long long> plus(P * (size_t)words), minus(P * (size_t)words);
  draws.assign(P, 0);
  if (want == Path::device && opt.has("device"))
    if (int rc = colate_set_device(std::stoi(opt.get("device")))) return api_error(rc), false;
  const long long cap = (long long)P * words;
  if (int rc = want == Path::device ? colate_topo::topo_view_device(v, cap, word_off.data(), plus.data(), minus.data(), draws.data())
                                    : colate_topo::topo_view_host(v, cap, word_off.data(), plus.data(), minus.data(), draws.data()))
    return api_error(rc), false;
  g_triple_stage_s = StageTimes::now() - t_stage;
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
  std::cerr << in.S << " samples staged, " << P << " triples drawn on the " << (want == Path::device ? "device" : "host") << std::endl;
  return true;
}

int run_topo_samples(const Options& opt) {
  for (const char* o : {"input", "pairs", "target_tmp", "reference_tmp", "target_mask", "reference_mask", "target_age", "reference_age", "bins", "coal",
                        "num_bootstraps", "ranks", "devices"})
    if (opt.has(o)) {
      std::cerr << "Error: --" << o << " cannot be combined with --mode count_topo --samples." << std::endl;
      return 1;
    }
  if (!opt.has("mut") || !opt.has("output")) {
    std::cerr << "Error: --samples needs --mut and -o PREFIX (optional: --chr, --seed, --device)." << std::endl;
    return 1;
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
  const unsigned seed = run_seed(opt);
  std::cerr << "---------------------------------------------------------" << std::endl;
  std::cerr << "Counting topologies for " << triples.size() << " triples.." << std::endl;
  Path want = Path::device;
  const char* e = std::getenv("COLATE_DEVICE_TOPO");
  if (e && std::string(e) == "0") {
    std::cerr << "triples drawn on the host (COLATE_DEVICE_TOPO=0)" << std::endl;
    want = Path::host_twin;
  } else if (colate_device_count() <= 0) {
    std::cerr << "triples drawn on the host (no device)" << std::endl;
    want = Path::host_twin;
  }
  const double t0 = StageTimes::now();
  WalkInputs in;
  std::vector<std::vector<TopoLine>> lines;
  std::vector<long long> draws;
  if (!draw_triples(opt, names, mut_files, triples, want, seed, in, lines, draws)) return 1;
  const double t1 = StageTimes::now();
  std::ofstream os(opt.get("output") + ".triples.txt");
  for (size_t p = 0; p < triples.size(); p++) {
    if (!write_lines(triples[p].output, names, lines[p])) return 1;
    long long plus = 0, minus = 0;
    for (const TopoLine& l : lines[p]) (l.sign > 0 ? plus : minus)++;
    os << triple_names[p] << " " << plus << " " << minus << " " << draws[p] << "\n";
  }
  os.close();
  if (!os) {
    std::cerr << "Error: cannot write " << opt.get("output") << ".triples.txt" << std::endl;
    return 1;
  }
  if (g_times.on)
    std::cerr << "Timing: count_topo samples: inputs " << t1 - t0 - g_triple_stage_s << " s, triple stage " << g_triple_stage_s << " s (device kernels "
              << colate_topo_samples_kernel_seconds() << " s), files " << StageTimes::now() - t1 << " s; " << (in.row_off.empty() ? 0LL : in.row_off.back())
              << " rows, " << in.S << " samples, " << triples.size() << " triples" << std::endl;
  print_usage_footer();
  return 0;
}

}  // namespace

int run_count_topo(const Options& opt) {
  if (opt.has("samples")) return run_topo_samples(opt);
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
  const unsigned seed = run_seed(opt);
  std::vector<std::string> names, mut_files;
  chromosome_files(opt, names, mut_files);
  PairSpec ps;
  ps.cond = opt.get("input"), ps.target = opt.get("target_tmp"), ps.reference = opt.get("reference_tmp"), ps.output = opt.get("output");
  const char* e = std::getenv("COLATE_DEVICE_TOPO");
  const Path want = e && std::string(e) == "1" ? Path::device : Path::cursors;
  WalkInputs in;
  std::vector<std::vector<TopoLine>> lines;
  std::vector<long long> draws;
  if (!draw_triples(opt, names, mut_files, std::vector<PairSpec>(1, ps), want, seed, in, lines, draws)) return 1;
  if (!write_lines(ps.output, names, lines[0])) return 1;
  print_usage_footer();
  return 0;
}

}  // namespace colate_drv
