// colate_amd/csrc/mut_interval.cpp -- `Colate --mode mut_interval`: interval-dated observations per genome block, read from
// a text file, through the block bootstrap and the EM fit (colate_bootstrap_em_interval_batch: both on the device, the
// weighted block sums never visit the host) to OUT.coal.  The reference has no such mode: it wrote and tested coal_EM for
// age_begin < age_end (coal_EM.cpp:153-468) but never put a loop around it; the driver follows mut() (coal.cpp:3071-3863)
// where the two overlap: epochs from --bins or --coal at age 0, the block weights of coal.cpp:3350-3357 from the run's
// std::mt19937, the reference's iteration limits, the .coal writer.
//
// How a line of the file becomes a mutation's (kind, age_begin, age_end) is the caller's business: the mode takes rows.
#include <unistd.h>

#include <cerrno>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <ctime>
#include <iostream>
#include <map>
#include <random>
#include <string>
#include <tuple>
#include <vector>

#include "colate_amd.h"
#include "mut_interval.h"

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

int run_mut_interval(const Options& opt) {
  if (!opt.has("rows") || !opt.has("output") || (!opt.has("bins") && !opt.has("coal"))) {
    std::cerr << "Error: --mode mut_interval needs --rows FILE, -o OUT and --bins x,y,stepsize or --coal FILE "
                 "(optional: --num_bootstraps, --seed, --years_per_gen, --max_iter, --min_iter, --device)."
              << std::endl;
    return 1;
  }
  std::cerr << "---------------------------------------------------------" << std::endl;
  std::cerr << "Calculating coalescence rates from interval-dated mutations.." << std::endl;
  double years_per_gen = 28.0;
  int B = 1, max_iter = COLATE_DEFAULT_MAX_ITER, min_iter = COLATE_DEFAULT_MIN_ITER;
  int seed = std::time(0) + getpid();  // coal.cpp:3158
  if (opt.has("years_per_gen")) years_per_gen = std::stof(opt.get("years_per_gen"));
  if (opt.has("seed")) seed = std::stoi(opt.get("seed"));
  if (opt.has("num_bootstraps")) B = std::stoi(opt.get("num_bootstraps"));
  if (opt.has("max_iter")) max_iter = std::stoi(opt.get("max_iter"));
  if (opt.has("min_iter")) min_iter = std::stoi(opt.get("min_iter"));
  if (B < 1) {
    std::cerr << "Error: --num_bootstraps must be at least 1." << std::endl;
    return 1;
  }
  auto api_error = [](int rc) {
    std::cerr << "Error: " << colate_last_error() << " (" << rc << ")" << std::endl;
    return 1;
  };

  // ---- epochs and starting rates, as for `mut` with a modern sample (coal.cpp:3501-3646)
  std::vector<double> epochs(COLATE_MAX_EPOCHS, 0.0), init_rates(COLATE_MAX_EPOCHS, COLATE_DEFAULT_INIT_RATE);
  int ep_null = 0;
  const int E = opt.has("coal") ? colate_epochs_from_coal(opt.get("coal").c_str(), 0.0, epochs.data(), init_rates.data(), COLATE_MAX_EPOCHS)
                                : colate_epochs_from_bins(opt.get("bins").c_str(), 0.0, years_per_gen, epochs.data(), COLATE_MAX_EPOCHS, &ep_null);
  if (E <= 0) {
    std::cerr << colate_last_error() << std::endl;
    return 1;
  }
  epochs.resize(E), init_rates.resize(E);

  // ---- the rows and the per-block tables
  IntervalRows rows;
  std::string err;
  if (!read_interval_rows(opt.get("rows"), epochs[0], rows, err)) {
    std::cerr << "Error: " << err << std::endl;
    return 1;
  }
  const int nb = rows.nb, R = rows.R;
  std::cerr << "Number of blocks: " << nb << std::endl;
  std::cerr << "Number of rows: " << R << std::endl;

  // ---- block weights (coal.cpp:3350-3357)
  std::mt19937 rng(seed);
  std::vector<double> weights((size_t)B * nb);
  if (int rc = colate_bootstrap_weights(&rng, B, nb, weights.data())) return api_error(rc);

  // ---- device or host twin
  std::string host_why;
  if (const char* e = std::getenv("COLATE_DEVICE_INTERVAL"))
    if (std::string(e) == "0") host_why = "COLATE_DEVICE_INTERVAL=0";
  if (host_why.empty() && colate_device_count() <= 0) host_why = "no device";
  if (host_why.empty() && opt.has("device"))
    if (int rc = colate_set_device(std::stoi(opt.get("device")))) return api_error(rc);

  std::cerr << "Maximising likelihood using EM.. " << std::endl;
  std::vector<double> rates((size_t)B * E), ll(B);
  std::vector<int> iters(B), flags(B);
  int rc;
  if (host_why.empty()) {
    rc = colate_bootstrap_em_interval_batch(B, nb, R, E, rows.kinds.data(), rows.age_begin.data(), rows.age_end.data(),
                                            weights.data(), rows.tables.data(), epochs.data(), init_rates.data(), max_iter,
                                            min_iter, COLATE_DEFAULT_REL_TOL, COLATE_DEFAULT_RATE_FLOOR, rates.data(),
                                            iters.data(), ll.data(), flags.data());
  } else {
    std::cerr << "interval fit on the host (" << host_why << ")" << std::endl;
    rc = colate_bootstrap_em_interval_batch_host(B, nb, R, E, rows.kinds.data(), rows.age_begin.data(), rows.age_end.data(),
                                                 weights.data(), rows.tables.data(), epochs.data(), init_rates.data(), max_iter,
                                                 min_iter, COLATE_DEFAULT_REL_TOL, COLATE_DEFAULT_RATE_FLOOR, rates.data(),
                                                 iters.data(), ll.data(), flags.data(), 1);
  }
  if (rc) return api_error(rc);
  for (int i = 0; i < B; i++) {
    std::cerr << "Bootstrap " << i + 1 << ": Total iterations " << iters[i] << std::endl;
    if (flags[i] & (COLATE_FLAG_NAN | COLATE_FLAG_NEG))
      std::cerr << "Warning: bootstrap " << i + 1 << " produced NaN or negative sufficient statistics." << std::endl;
  }
  if (colate_write_coal((opt.get("output") + ".coal").c_str(), B, E, epochs.data(), rates.data(), 0, ep_null)) {
    std::cerr << "Error: " << colate_last_error() << std::endl;
    return 1;
  }
  print_usage_footer();
  return 0;
}

}  // namespace colate_drv
