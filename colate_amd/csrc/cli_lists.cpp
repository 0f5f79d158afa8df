// colate_amd/csrc/cli_lists.cpp -- the list front end and the per-pair run back end of the `Colate` drivers (cli_lists.h): what
// `--mode mut`, `mut_interval`, `compare_tmp` and `count_topo` say and check in the same words, in one place.
#include <unistd.h>

#include <cstdio>
#include <ctime>
#include <iostream>
#include <sstream>

#include "cli_lists.h"
#include "colate_amd.h"

namespace colate_drv {

// ------------------------------------------------------------------ the list front end
// the whole token as std::stof reads it; false where it is no number
static bool parse_age(const std::string& tok, float& v) {
  size_t used = 0;
  try {
    v = std::stof(tok, &used);
  } catch (...) {
    return false;
  }
  return used != 0 && used == tok.size();
}

bool read_pair_list(const std::string& path, const Options& opt, const std::vector<std::string>& chr_names, std::vector<PairSpec>& pairs) {
  std::ifstream is(path);
  if (!is) {
    std::cerr << "Error while opening file " << path << std::endl;
    return false;
  }
  std::string line;
  for (size_t line_no = 1; std::getline(is, line); line_no++) {
    std::istringstream ss(line);
    PairSpec ps;
    if (!(ss >> ps.target >> ps.reference >> ps.output)) continue;
    auto fail = [&](const std::string& what) {
      std::cerr << "Error: " << path << ", line " << line_no << ": " << what << std::endl;
      return false;
    };
    int n_ages = 0;
    bool seen_tm = false, seen_rm = false, seen_coal = false;
    for (std::string tok; ss >> tok;) {
      const size_t eq = tok.find('=');
      if (eq == std::string::npos) {
        if (n_ages == 2) return fail("more than two ages ('" + tok + "')");
        float v = 0;
        if (!parse_age(tok, v)) return fail("the age '" + tok + "' is not a number");
        (n_ages++ == 0 ? ps.target_age : ps.ref_age) = v;
        continue;
      }
      const std::string key = tok.substr(0, eq), value = tok.substr(eq + 1);
      bool* seen = key == "target_mask" ? &seen_tm : key == "reference_mask" ? &seen_rm : key == "coal" ? &seen_coal : nullptr;
      if (!seen) return fail("unknown key '" + key + "' (known: target_mask, reference_mask, coal)");
      if (*seen) return fail("the key '" + key + "' is given twice");
      if (value.empty()) return fail("the key '" + key + "' has no value");
      *seen = true;
      if (key == "target_mask") ps.target_masks = mask_files(opt, chr_names, value);
      else if (key == "reference_mask") ps.ref_masks = mask_files(opt, chr_names, value);
      else ps.coal = value;
    }
    ps.line = line_no, ps.ages_given = n_ages;
    pairs.push_back(ps);
  }
  if (pairs.empty()) {
    std::cerr << "Error: no pairs in " << path << std::endl;
    return false;
  }
  return true;
}

bool read_sample_list(const std::string& path, const Options& opt, const std::vector<std::string>& chr_names, bool with_ages,
                      std::vector<SampleLine>& samples, bool with_cond) {
  std::ifstream is(path);
  if (!is) {
    std::cerr << "Error while opening file " << path << std::endl;
    return false;
  }
  std::string line;
  for (size_t line_no = 1; std::getline(is, line); line_no++) {
    auto fail = [&](const std::string& what) {
      std::cerr << "Error: " << path << ", line " << line_no << ": " << what << std::endl;
      return false;
    };
    std::istringstream ss(line);
    SampleLine sl;
    sl.line = line_no, sl.cond = with_cond;
    if (!(ss >> sl.name)) continue;  // a blank line
    if (sl.name.find('=') != std::string::npos) return fail("the line starts with '" + sl.name + "': the sample's NAME is missing or empty");
    if (sl.name.find('/') != std::string::npos) return fail("the NAME '" + sl.name + "' contains '/'");
    if (!(ss >> sl.file) || sl.file.find('=') != std::string::npos)
      return fail(with_ages ? "expected `NAME FILE.colate.in [mask=PREFIX] [role=target|reference] [age=YEARS]`"
                            : "expected `NAME FILE.colate.in [mask=PREFIX] [role=target|reference]`");
    for (const SampleLine& other : samples)
      if (other.name == sl.name) return fail("the NAME '" + sl.name + "' is given twice (first on line " + std::to_string(other.line) + ")");
    bool seen_mask = false, seen_role = false, seen_age = false;
    for (std::string tok; ss >> tok;) {
      const size_t eq = tok.find('=');
      if (eq == std::string::npos)
        return fail("'" + tok + "' is no key=value token (" +
                    (with_ages ? "a sample's age is given as age=YEARS)" : "--mode mut_interval takes modern samples only: a line cannot carry sample ages)"));
      const std::string key = tok.substr(0, eq), value = tok.substr(eq + 1);
      bool* seen = key == "mask" ? &seen_mask : key == "role" ? &seen_role : (with_ages && key == "age") ? &seen_age : nullptr;
      if (!seen) return fail("unknown key '" + key + (with_ages ? "' (known: mask, role, age)" : "' (known: mask, role)"));
      if (*seen) return fail("the key '" + key + "' is given twice");
      if (value.empty()) return fail("the key '" + key + "' has no value");
      *seen = true;
      if (key == "mask") sl.masks = mask_files(opt, chr_names, value);
      else if (key == "age") {  // (read as the ages of a `--pairs` line are)
        float v = 0;
        if (!parse_age(value, v) || !(v == v)) return fail("the age '" + value + "' is not a number");
        if (v < 0) return fail("the age '" + value + "' is negative");
        sl.age = v;
      } else if (with_cond) {  // (`--mode count_topo`: a comma-separated subset of the three roles)
        sl.cond = sl.target = sl.reference = false;
        std::istringstream roles(value);
        for (std::string r; std::getline(roles, r, ',');) {
          bool* const on = r == "cond" ? &sl.cond : r == "target" ? &sl.target : r == "reference" ? &sl.reference : nullptr;
          if (!on) return fail("unknown role '" + r + "' (known: cond, target, reference)");
          if (*on) return fail("the role '" + r + "' is given twice");
          *on = true;
        }
      } else if (value == "target") sl.reference = false;
      else if (value == "reference") sl.target = false;
      else return fail("unknown role '" + value + "' (known: target, reference)");
    }
    samples.push_back(sl);
  }
  bool any_t = false, any_r = false, any_c = !with_cond;
  for (const SampleLine& sl : samples) any_t = any_t || sl.target, any_r = any_r || sl.reference, any_c = any_c || sl.cond;
  if (!any_c) {
    std::cerr << "Error: " << path << ": the list names no cond sample." << std::endl;
    return false;
  }
  if (!any_t || !any_r) {
    std::cerr << "Error: " << path << ": the list names no " << (!any_t ? "target" : "reference") << " sample." << std::endl;
    return false;
  }
  return true;
}

bool sample_pairs(const std::vector<SampleLine>& samples, const std::string& prefix, const std::string& list, std::vector<PairSpec>& pairs) {
  for (const SampleLine& t : samples)
    for (const SampleLine& r : samples) {
      if (!t.target || !r.reference || &t == &r) continue;
      PairSpec ps;
      ps.target = t.file, ps.reference = r.file, ps.output = prefix + "_" + t.name + "_" + r.name;
      ps.target_age = t.age, ps.ref_age = r.age, ps.target_masks = t.masks, ps.ref_masks = r.masks, ps.line = t.line;
      ps.target_name = t.name, ps.ref_name = r.name;
      pairs.push_back(ps);
    }
  if (pairs.empty()) std::cerr << "Error: " << list << ": no pair of a target and a reference on different lines." << std::endl;
  return !pairs.empty();
}

bool pairs_have_epochs(const Options& opt, const std::vector<PairSpec>& pairs) {
  for (size_t p = 0; p < pairs.size(); p++)
    if (!opt.has("bins") && pairs[p].coal.empty()) {  // (a line with coal= takes its epochs from that file)
      std::cerr << "Error: --pairs needs --bins for pair " << p + 1 << " (it names no coal= file)." << std::endl;
      return false;
    }
  return true;
}

bool refuse_options(const Options& opt, std::initializer_list<const char*> names, const std::string& what) {
  for (const char* o : names)
    if (opt.has(o)) {
      std::cerr << "Error: --" << o << " cannot be combined with " << what << "." << std::endl;
      return true;
    }
  return false;
}
bool refuse_per_line_options(const Options& opt) {
  for (const char* o : {"target_mask", "reference_mask", "coal"})
    if (refuse_options(opt, {o}, std::string("--pairs (give it per line: ") + o + "=...)")) return true;
  return false;
}

Path choose_path(const char* env, bool list, std::string& why) {
  const char* e = env ? std::getenv(env) : nullptr;
  if (!list) return e && std::string(e) == "1" ? Path::device : Path::cursors;
  if (e && std::string(e) == "0") why = std::string(env) + "=0";
  else if (colate_device_count() <= 0) why = "no device";
  return why.empty() ? Path::device : Path::host_twin;
}
bool bind_device(const Options& opt) {
  if (!opt.has("device")) return true;
  const int rc = colate_set_device(opt.get_int("device"));
  if (rc) api_error(rc);
  return !rc;
}

bool check_readable(const std::vector<const std::string*>& files, const char* lead) {
  for (const std::string* f : files) {
    FILE* fp = std::fopen(f->c_str(), "rb");
    if (!fp) {
      std::cerr << "Error: " << lead << " " << *f << std::endl;
      return false;
    }
    std::fclose(fp);
  }
  return true;
}
bool close_checked(std::ofstream& os, const std::string& path) {
  os.close();
  if (!os) std::cerr << "Error: cannot write " << path << std::endl;
  return !!os;
}

// ------------------------------------------------------------------ the per-pair run back end
bool RunOptions::read_replicates(const Options& opt, bool with_iters) {
  seed = run_seed(opt);  // one seed for the whole run
  if (opt.has("num_bootstraps")) B = opt.get_int("num_bootstraps");
  if (with_iters && opt.has("max_iter")) max_iter = opt.get_int("max_iter");
  if (with_iters && opt.has("min_iter")) min_iter = opt.get_int("min_iter");
  if (B < 1) std::cerr << "Error: --num_bootstraps must be at least 1." << std::endl;
  return B >= 1;
}

int run_seed(const Options& opt) { return opt.has("seed") ? opt.get_int("seed") : (int)(std::time(nullptr) + getpid()); }

int epochs_for(const Options& opt, const std::string* coal, double age, double years_per_gen, std::vector<double>& epochs,
               std::vector<double>& init, int& ep_null) {
  epochs.assign(COLATE_MAX_EPOCHS, 0.0);
  init.assign(COLATE_MAX_EPOCHS, COLATE_DEFAULT_INIT_RATE);
  ep_null = 0;
  const int E = coal ? colate_epochs_from_coal(coal->c_str(), age, epochs.data(), init.data(), COLATE_MAX_EPOCHS)
                     : colate_epochs_from_bins(opt.get("bins").c_str(), age, years_per_gen, epochs.data(), COLATE_MAX_EPOCHS, &ep_null);
  if (E > 0) epochs.resize(E), init.resize(E);
  return E;
}

std::vector<std::vector<size_t>> classes_by_epoch_count(const std::vector<std::vector<double>>& epochs, const std::vector<char>* usable) {
  std::vector<std::vector<size_t>> classes;
  for (size_t p = 0; p < epochs.size(); p++) {
    if (usable && !(*usable)[p]) continue;
    size_t c = 0;
    while (c < classes.size() && epochs[classes[c][0]].size() != epochs[p].size()) c++;
    if (c == classes.size()) classes.emplace_back();
    classes[c].push_back(p);
  }
  return classes;
}

void report_bootstraps(int pair, int B, int E, const int* iters, const int* flags, bool as_mut) {
  const std::string p = std::to_string(pair);
  int unresolved_max = 0;
  for (int i = 0; i < B; i++) {
    std::cerr << (pair ? "Pair " + p + " " : "") << "Bootstrap " << i + 1 << ": Total iterations " << iters[i] << std::endl;
    if (flags[i] & (COLATE_FLAG_NAN | COLATE_FLAG_NEG))
      std::cerr << "Warning: " << (pair ? "pair " + p + " " : "") << "bootstrap " << i + 1 << " produced NaN or negative sufficient statistics"
                << (as_mut ? " (the reference aborts here)." : ".") << std::endl;
    unresolved_max = std::max(unresolved_max, COLATE_UNRESOLVED_EPOCHS(flags[i]));
  }
  if (as_mut && unresolved_max > 0)  // (include/colate_amd.h, COLATE_FLAG_UNRESOLVED)
    std::cerr << "Note: " << (pair ? "pair " + p + ": " : "") << "the last " << unresolved_max << " of " << E
              << " epochs are older than the data resolve: "
              << "their printed rates depend on rounding residue (in the reference build too) and are not reproducible."
              << std::endl;
}

void say_blocks(size_t p, size_t P, const PairSpec& ps, int nb) {
  std::cerr << "Pair " << p + 1 << " / " << P << ": " << ps.target << " x " << ps.reference << ": Number of blocks: " << nb << std::endl;
}

bool write_coal(const std::string& stem, int B, int E, const double* epochs, const double* rates, bool is_ancient, int ep_null) {
  const int rc = colate_write_coal((stem + ".coal").c_str(), B, E, epochs, rates, is_ancient ? 1 : 0, ep_null);
  if (rc) std::cerr << "Error: " << colate_last_error() << std::endl;
  return !rc;
}

}  // namespace colate_drv
