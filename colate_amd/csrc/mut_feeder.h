// colate_amd/csrc/mut_feeder.h -- what the host-side translation units of the `Colate --mode mut` driver share: mut_driver.cpp
// (command line, readers, the sequential feeder of include/coal/coal.cpp:2071-2321, the single-pair, --pairs and --samples
// drivers around mut(), --ranks launcher), mut_pairs.cpp (the table-fill engine of the batched front end, SURVEY.md section 8
// f2 / BASELINE configs[4], which fills every table of a `--pairs` run and of a single pair, and hands a pair it cannot fill
// exactly to the sequential feeder) and fill_samples.cpp (the fill of a `--samples` run on the device, which falls back to that
// engine).  The age bins and the uniform stream of the fills are in age_bins.hpp and uniform_stream.hpp.
#pragma once
#include <zlib.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <functional>
#include <map>
#include <memory>
#include <random>
#include <sstream>
#include <string>
#include <vector>

#include "colate_amd.h"

namespace colate_drv {

struct Options {
  std::map<std::string, std::string> kv;
  bool has(const std::string& k) const { return kv.count(k) > 0; }
  const std::string& get(const std::string& k) const { return kv.at(k); }
};

// stage timing (COLATE_TIMING=1: one stderr line at the end)
struct StageTimes {
  double parse_mut = 0, table_fill = 0, bootstrap_em = 0;
  bool on = std::getenv("COLATE_TIMING") != nullptr;
  static double now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
};
extern StageTimes g_times;

// igzstream semantics of the reference: zlib reads gzip and plain files alike.
class GzText {
 public:
  bool open(const std::string& name) {
    close();
    f_ = gzopen(name.c_str(), "rb");
    if (f_) gzbuffer(f_, 1 << 20);
    return f_ != nullptr;
  }
  bool is_open() const { return f_ != nullptr; }
  bool getline(std::string& line) {
    line.clear();
    if (!f_) return false;
    char buf[1 << 14];
    bool got = false;
    while (gzgets(f_, buf, sizeof(buf))) {
      got = true;
      size_t n = std::strlen(buf);
      if (n && buf[n - 1] == '\n') {
        line.append(buf, n - 1);
        return true;
      }
      line.append(buf, n);
    }
    return got;
  }
  void close() {
    if (f_) gzclose(f_);
    f_ = nullptr;
  }
  ~GzText() { close(); }

 private:
  gzFile f_ = nullptr;
};

// Only the columns parse_tmptmp looks at (mutations.cpp:77-246):
// snp;pos;dist;rs;tree;branches;is_not_mapping;is_flipped;age_begin;age_end;anc/der;...
struct MutRow {
  int pos = 0;
  int dist = 0, tree = 0;  // (CondCoalRates: the tree weights, mutations.cpp:616-670)
  int num_branches = 0;
  int flipped = 0;
  float age_begin = 0.0f, age_end = 0.0f;  // stored as float in the reference (mutations.hpp:21)
  std::string mutation_type = "NA";
};
// the rows of one .mut(.gz) file (mutations.cpp:56-283); exits like the reference when the file cannot be read
bool read_mut_file(const std::string& filename, std::vector<MutRow>& rows);
// the same, row by row (nothing is kept)
bool for_each_mut_row(const std::string& filename, const std::function<void(const MutRow&)>& sink);
// the upper-cased sequence of a fasta mask (data.cpp:213-235); exits like the reference when the file cannot be opened
void read_fasta_mask(const std::string& filename, std::string& seq);
// ... only the opening (and its exit)
void check_fasta_mask(const std::string& filename);

struct PairTables {  // flat [nb][A] tables of one pair, as the bootstrap takes them; she / nse = row 0 of the reference's A*A tables
  int nb = 0;
  std::vector<double> sh, ns, she, nse;
  std::mt19937 rng;  // the run's generator after the table fill
  // the four tables from `blocks` blocks of [4][A] in the order of the fill (sh | ns | she | nse); block(j): block j's
  template <class BlockAt>
  void set_blocks(int blocks, int A, BlockAt block) {
    nb = blocks;
    std::vector<double>* const tab[4] = {&sh, &ns, &she, &nse};
    for (int k = 0; k < 4; k++) {
      tab[k]->resize((size_t)nb * A);
      for (int j = 0; j < nb; j++) std::copy_n(block(j) + (size_t)k * A, A, tab[k]->begin() + (size_t)j * A);
    }
  }
};

// `--ranks N`: this process is rank `rank` of `nranks` (run_ranked forks them); the 128-byte RCCL id travels from
// rank 0 to the others through the launcher's pipes.
struct RankCtx {
  bool ranked = false;  // launched by run_ranked (also with one rank: the RCCL path with a communicator of one)
  int rank = 0, nranks = 1;
  int fd_id_out = -1;  // rank 0: writes the id here
  int fd_id_in = -1;   // ranks > 0: read it here
};
extern RankCtx g_rank;
bool write_all(int fd, const void* buf, size_t n);
bool read_all(int fd, void* buf, size_t n);

struct PairSpec {
  std::string target, reference, output;
  double target_age = 0, ref_age = 0;
  std::vector<std::string> target_masks, ref_masks;  // one fasta per chromosome, or none
  std::string coal;                                   // --pairs `coal=FILE`: the pair's epochs and starting rates ("": --bins)
  std::string cond;                                   // `--mode count_topo`: the conditioning sample's file ("": every other mode)
  size_t line = 0;                                    // --pairs: the line of the list (1-based), and how many ages it carried
  int ages_given = 0;
};

// coal.cpp:2071-2321 for one (target, reference) pair, on the calling thread in the reference's order: the sequential feeder.
// Fills tab.sh, ns, she, nse and tab.nb (not tab.rng: the draws come from `rng`).  Returns the number of genome blocks.
int fill_tables_from_tmp(const std::vector<std::string>& chr_names, const std::vector<std::string>& mut_files,
                         const std::string& target_file, const std::string& ref_file,
                         const std::vector<std::string>& target_masks, const std::vector<std::string>& ref_masks, double C,
                         std::mt19937& rng, int num_bases_per_block, int A, PairTables& tab);

// the chromosome list of --chr (coal.cpp:3295-3310): names, <mut>_chr<name>.mut paths and, where asked for and given,
// <mask>_chr<name>.fa paths of --target_mask / --reference_mask; without --chr one unnamed chromosome and the paths verbatim
void chromosome_files(const Options& opt, std::vector<std::string>& names, std::vector<std::string>& mut_files,
                      std::vector<std::string>* target_masks = nullptr, std::vector<std::string>* ref_masks = nullptr);
// the fasta files of one mask PREFIX over those chromosomes: PREFIX_chr<name>.fa each with --chr, else PREFIX itself
std::vector<std::string> mask_files(const Options& opt, const std::vector<std::string>& names, const std::string& prefix);

void write_counts_file(const std::string& path, int B, int A, const std::vector<double>& grid, const double* csh,
                       const double* cns);
void print_usage_footer();
void print_help();  // mut_driver.cpp: the option list
// condcoal.cpp: `--mode CondCoalRates`
int run_condcoal(const Options& opt);  // "CPU Time spent: ...; Max Memory usage: ..." (coal.cpp:3852-3861)

// mut_pairs.cpp: the engine.  The tables of the pairs listed in `todo` (indices into `pairs`; the others stay empty) and
// each pair's generator as the fill leaves it; `names` / `mut_files`: the chromosomes (chromosome_files).  False after an
// error message.
bool fill_pairs(const Options& opt, const std::vector<std::string>& names, const std::vector<std::string>& mut_files,
                const std::vector<PairSpec>& pairs, const std::vector<size_t>& todo, int seed, int A, std::vector<PairTables>& out);
// fill_samples.cpp: the same for the pairs of a `--samples` list.  Where there is a device and every sample has a walk index,
// no pair is walked on the host: the index arrays and the rows go to the device once, and colate_fill_samples' device form
// walks, forms the records and fills the tables there (fill_samples.h).  Otherwise one line on stderr says why, and the pairs
// go through fill_pairs.
bool fill_sample_pairs(const Options& opt, const std::vector<std::string>& names, const std::vector<std::string>& mut_files,
                       const std::vector<PairSpec>& pairs, const std::vector<size_t>& todo, int seed, int A, std::vector<PairTables>& out);
// mut_driver.cpp: a failed C-ABI call: "Error: <the library's message> (<rc>)"; returns the exit code
int api_error(int rc);

// mut_pairs.cpp: the engine's walk for `--mode mut_interval`.  The SNPs the pair uses -- use filter, block advance, masks and
// the float rounding of the target genotype are those of fill_pairs, coal.cpp:2148-2244 -- as interval-dated observations
// (interval_cells.h) in the walk's order: chromosome, then file order; blocks[i]: the genome block of record i, numbered
// as fill_pairs numbers them; nb: the number of genome blocks.  Nothing is drawn.  False after an error message.
bool collect_interval_records(const std::vector<std::string>& names, const std::vector<std::string>& mut_files, const PairSpec& pair,
                              std::vector<colate_interval_rec>& recs, std::vector<int>& blocks, int& nb);
// The same for a list of pairs (`--mode mut_interval --pairs`): every .mut file, .colate.in file and mask is read and decoded
// once (the inputs of fill_pairs), the pairs are walked on the pool, and out[p] holds pair p's records and blocks in its
// walk's order -- what collect_interval_records gives for that pair alone, which is this function on a list of one.
// walked: false where the pair's walk did not finish.  False after an error message.
struct PairRecords {
  std::vector<colate_interval_rec> recs;
  std::vector<int> blocks;
  int nb = 0;
  bool walked = false;
};
bool collect_interval_records_pairs(const std::vector<std::string>& names, const std::vector<std::string>& mut_files,
                                    const std::vector<PairSpec>& pairs, std::vector<PairRecords>& out);

// mut_pairs.cpp: the inputs of a list of pairs as the pair walk over walk indices takes them (`--mode mut_interval --samples`;
// csrc/interval_walk.h): every .mut file, .colate.in file and mask read, decoded and indexed once by the loader of fill_pairs.
// indexed: every file has a walk index -- only then are the arrays below filled.  The rows of all chromosomes back to back;
// per (sample, chromosome) the file's index where it lies, per (mask, chromosome) the mask's bits; samples are the distinct
// .colate.in paths, masks the distinct lists of mask files, both in the order of their names.  The object owns what it points to.
constexpr int kIntervalBasesPerBlock = (int)30e6;  // the genome block of `--mode mut_interval` (coal.cpp: num_bases_per_block)
// `--mode compare_tmp`: what the raw rows of a chromosome's .mut file decide (csrc/compare_tmp.h: the windows)
struct CompareChromosome {
  int first_pos = 0, last_pos = 0;  // the file's first and last raw rows
  size_t raw_rows = 0;
  bool ascend = true;           // no raw row lies below the one in front
  int windows = 1;              // lines the chromosome prints
  std::vector<int> row_window;  // per searched row: the lines printed in front of it
};
struct WalkInputs {
  struct Loaded;
  std::unique_ptr<Loaded> loaded;
  bool indexed = false;
  std::vector<long long> row_off;
  std::vector<colate_walk_row> rows;
  std::vector<const colate_walk_row*> row_ptrs;            // [C]
  std::vector<const colate_walk_idx*> idx_ptrs;            // [S][C]
  std::vector<const unsigned long long*> mask_ptrs;        // [M][C]
  std::vector<colate_walk_pair> pairs;
  std::vector<const colate_walk_idx*> cidx_ptrs;           // [S][C]: the cond indices, with RowSet::count_topo only
  std::vector<int> cond_ids;                               // [P]: the sample id of every pair's `cond` file
  int S = 0, M = 0;
  std::vector<CompareChromosome> compare;  // [C], with RowSet::compare_tmp only
  bool files_ok = false;                   // every .colate.in file could be opened
  WalkInputs();
  ~WalkInputs();
};
enum class RowSet { mut, compare_tmp, count_topo };  // whose row filter the loader applies
bool load_walk_inputs(const std::vector<std::string>& names, const std::vector<std::string>& mut_files, const std::vector<PairSpec>& pairs,
                      WalkInputs& out, RowSet set = RowSet::mut);
// RowSet::compare_tmp: the rows kept are those of that mode's filter (compact rows without age_end >= 0), `compare` is filled, and
// `indexed` also says that no chromosome's raw rows descend.
// RowSet::count_topo: the rows of that mode's filter (age_begin <= age_end, no age_end >= 0); every pair's `cond` file is loaded
// with the other two, every file gets a cond index next to its walk index, and cidx_ptrs / cond_ids are filled.
// mut_pairs.cpp: the cursor walk of `--mode count_topo` (count_topo.h: cursor_walk_chromosome) for every triple of a list over
// inputs loaded with RowSet::count_topo, each triple drawing from its own std::mt19937 on `seed`: the lines a triple prints, in
// order, and its qualifying rows.  Right for every input; false without loaded inputs.
struct TopoLine {
  int chr, pos;
  float age_begin, age_end;
  int sign, DAF, N;  // the conditioning record's counts
};
// profile (`--age_profile`): epochs[E] in, counts[P][E][3] out -- per triple and epoch (count_topo.h: age_epoch) the rows printed
// with +1, with -1, and the qualifying rows.
struct TopoProfile {
  int E = 0;
  const double* epochs = nullptr;
  std::vector<long long> counts;
};
bool topo_cursor_triples(const WalkInputs& loaded, const std::vector<std::string>& names, const std::vector<PairSpec>& triples, unsigned seed,
                         std::vector<std::vector<TopoLine>>& lines, std::vector<long long>& draws, TopoProfile* profile = nullptr);
// topo_driver.cpp: `Colate --mode count_topo`
int run_count_topo(const Options& opt);
// mut_pairs.cpp: the cursor walk of `--mode compare_tmp` (compare_tmp.h: cursor_walk_chromosome) for every pair of a list over inputs
// loaded with RowSet::compare_tmp: mismatch / snps [P][sum of compare[c].windows].  Right for every input; false without loaded inputs.
bool compare_cursor_pairs(const WalkInputs& loaded, const std::vector<std::string>& names, const std::vector<PairSpec>& pairs,
                          std::vector<int>& mismatch, std::vector<int>& snps);
// compare_driver.cpp: `Colate --mode compare_tmp`
int run_compare_tmp(const Options& opt);
// collect_interval_records_pairs on inputs loaded before (the path `--samples` takes where a file has no walk index)
bool collect_interval_records_loaded(const WalkInputs& loaded, const std::vector<std::string>& names, const std::vector<PairSpec>& pairs,
                                     std::vector<PairRecords>& out);

// mut_driver.cpp: the list of `--pairs`.  "target reference output [target_age [reference_age]]" per line; after the three
// names, `key=value` tokens in any order and mixed with the ages: target_mask=PREFIX, reference_mask=PREFIX (expanded as the
// single-pair CLI expands --target_mask / --reference_mask: with --chr PREFIX_chr<name>.fa per chromosome, else PREFIX itself)
// and coal=FILE (the pair's warm start).  A token with '=' is a key, any other the next age.  An unknown, repeated or empty key,
// a third age or an age that is no number is an error naming the file and the line.  A line of fewer than three tokens is
// skipped.  PairSpec::line / ages_given: the pair's line in the file and how many age tokens it carried.
bool read_pair_list(const std::string& path, const Options& opt, const std::vector<std::string>& chr_names, std::vector<PairSpec>& pairs);

// mut_driver.cpp: the list of `--samples` (both `--mode mut` and `--mode mut_interval`).  `NAME FILE.colate.in` per line, then
// in any order mask=PREFIX (expanded as --target_mask is), role=target|reference (default: both) and -- with_ages only, which
// `--mode mut` passes -- age=YEARS, the sample's age (default 0; a number, not negative).  Blank lines are skipped.  Every error
// names the line.  The pairs of a list are every (target line, reference line) of different lines, targets outermost.
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
// mut_driver.cpp: `Colate --mode mut --samples LIST`
int run_mut_samples(const Options& opt);

}  // namespace colate_drv
