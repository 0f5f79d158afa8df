// colate_amd/csrc/cli_lists.h -- what the drivers of `Colate` share around their modes (cli_lists.cpp), written once:
//   * the list front end of `--pairs` and `--samples`: the two list readers, the refusal of options a list mode cannot take, a
//     sample list as pairs, the choice between device, host twin and cursors, and the small file checks;
//   * the per-pair run back end of `--mode mut` and `--mode mut_interval`: the run's options, a pair's epochs and starting rates,
//     the classes of pairs with the same number of epochs, and what is said per pair and per bootstrap.
#pragma once
#include <fstream>
#include <initializer_list>
#include <string>
#include <vector>

#include "cli_options.h"
#include "colate_amd.h"
#include "mut_inputs.h"

namespace colate_drv {

// ------------------------------------------------------------------ the list front end
// The list of `--pairs`.  "target reference output [target_age [reference_age]]" per line; after the three names, `key=value` tokens
// in any order and mixed with the ages: target_mask=PREFIX, reference_mask=PREFIX (expanded as the single-pair CLI expands
// --target_mask / --reference_mask: with --chr PREFIX_chr<name>.fa per chromosome, else PREFIX itself) and coal=FILE (the pair's warm
// start).  A token with '=' is a key, any other the next age.  An unknown, repeated or empty key, a third age or an age that is no
// number is an error naming the file and the line.  A line of fewer than three tokens is skipped.  PairSpec::line / ages_given: the
// pair's line in the file and how many age tokens it carried.
bool read_pair_list(const std::string& path, const Options& opt, const std::vector<std::string>& chr_names, std::vector<PairSpec>& pairs);

// The list of `--samples`.  `NAME FILE.colate.in` per line, then in any order mask=PREFIX (expanded as --target_mask is),
// role=target|reference (default: both) and -- with_ages only, which `--mode mut` passes -- age=YEARS, the sample's age (default 0; a
// number, not negative).  Blank lines are skipped.  Every error names the line.  The pairs of a list are every (target line,
// reference line) of different lines, targets outermost.
struct SampleLine {
  std::string name, file;
  std::vector<std::string> masks;
  bool target = true, reference = true;
  bool cond = false;  // with_cond only (default there: all three roles)
  double age = 0;
  size_t line = 0;
};
// with_cond (`--mode count_topo` only): role= takes a comma-separated subset of cond,target,reference (default: all three), and a
// list without a cond sample is an error; every other mode refuses role=cond as an unknown role.
bool read_sample_list(const std::string& path, const Options& opt, const std::vector<std::string>& chr_names, bool with_ages,
                      std::vector<SampleLine>& samples, bool with_cond = false);
// Those pairs, each with what its two lines know: files, PREFIX_<target>_<reference> as output, ages, masks, the target's line and
// the two names.  False after the error message of a list without a pair (`list`: its path).
bool sample_pairs(const std::vector<SampleLine>& samples, const std::string& prefix, const std::string& list, std::vector<PairSpec>& pairs);

// Every line of a `--pairs` list has its epochs: --bins, or its own coal= file.  False after the error message.
bool pairs_have_epochs(const Options& opt, const std::vector<PairSpec>& pairs);

// True after "Error: --<o> cannot be combined with <what>." for the first of `names` that was given ...
bool refuse_options(const Options& opt, std::initializer_list<const char*> names, const std::string& what);
// ... and for the three options that a `--pairs` list takes per line: one mask / one warm start cannot mean the same for a whole
// list of pairs: refuse, do not ignore
bool refuse_per_line_options(const Options& opt);

// Where a stage runs: on the record cursors of the reference, on the host twin of the kernels, or on the device.  A list run
// (`list`) takes the device unless COLATE_DEVICE_<X> (`env`, or none) is 0 or there is no device, and then the host twin, `why`
// saying which; a single run takes the cursors unless the variable is 1.  The callers say it in their own words.
enum class Path { cursors, host_twin, device };
Path choose_path(const char* env, bool list, std::string& why);
// --device N: this process's GPU.  False after the library's message.
bool bind_device(const Options& opt);

// Every file can be opened; else false after "Error: <lead> <file>" for the first that cannot.
bool check_readable(const std::vector<const std::string*>& files, const char* lead);
// Closes the written file; false after "Error: cannot write <path>" where a write or the close failed.
bool close_checked(std::ofstream& os, const std::string& path);

// ------------------------------------------------------------------ the per-pair run back end
// --years_per_gen at once; then (read_replicates, false after the error message) the seed of the run's generators -- --seed, else
// time plus pid (coal.cpp:3158) --, the number of bootstrap replicates and, for `--mode mut_interval` (with_iters), the limits of
// the EM, which are the reference's where they are not read.  Two steps: the single pair of `--mode mut` speaks in between.
struct RunOptions {
  double years_per_gen = 28.0;
  int seed = 0, B = 1, max_iter = COLATE_DEFAULT_MAX_ITER, min_iter = COLATE_DEFAULT_MIN_ITER;
  explicit RunOptions(const Options& opt) {
    if (opt.has("years_per_gen")) years_per_gen = opt.get_float("years_per_gen");
  }
  bool read_replicates(const Options& opt, bool with_iters);
};
int run_seed(const Options& opt);  // --seed, else time plus pid (coal.cpp:3158, 4545-4549)
// A pair's epochs and starting rates (coal.cpp:3501-3646): from the .coal file `coal` (which gives the rates too; ep_null 0)
// or, without one, from --bins and the pair's age.  Returns E, the two vectors sized to it, or <= 0 (colate_last_error(): the
// caller leads it in).
int epochs_for(const Options& opt, const std::string* coal, double age, double years_per_gen, std::vector<double>& epochs,
               std::vector<double>& init, int& ep_null);
// classes of pairs with the same number of epochs, in order of first appearance (usable: where given, the pairs that count)
std::vector<std::vector<size_t>> classes_by_epoch_count(const std::vector<std::vector<double>>& epochs, const std::vector<char>* usable = nullptr);
// The lines of one pair's B replicates.  `pair`: the pair's number in a list, which then leads each line; 0 for a single pair.
// as_mut (`--mode mut`, where the reference has the loop): the warning says what the reference does, and the last of the E epochs
// that the data do not resolve are noted.
void report_bootstraps(int pair, int B, int E, const int* iters, const int* flags, bool as_mut);
void say_blocks(size_t p, size_t P, const PairSpec& ps, int nb);
// <stem>.coal: the epochs and a pair's [B][E] rates (colate_write_coal); false after the library's message
bool write_coal(const std::string& stem, int B, int E, const double* epochs, const double* rates, bool is_ancient, int ep_null);

}  // namespace colate_drv
