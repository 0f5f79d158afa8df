// colate_amd/csrc/mut_inputs.h -- the readers and the inputs of the `Colate` drivers: the .mut, fasta and --chr readers and the
// sequential feeder of include/coal/coal.cpp:2071-2321 (mut_readers.cpp), a pair as the drivers name it and its tables, and the
// fills that turn pairs into tables: the engine of the batched front end (mut_pairs.cpp; SURVEY.md section 8 f2 / BASELINE
// configs[4]), which fills every table of a `--pairs` run and of a single pair and hands a pair it cannot fill exactly to the
// sequential feeder, and the fill of a `--samples` run on the device, which falls back to that engine (fill_samples.cpp).  The age
// bins and the uniform stream of the fills are in age_bins.hpp and uniform_stream.hpp.
#pragma once
#include <zlib.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <random>
#include <string>
#include <vector>

#include "cli_options.h"

namespace colate_drv {

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
  std::string read_all() {  // the rest of the file, every line ended by a newline
    std::string all, line;
    while (getline(line)) all += line + '\n';
    return all;
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

struct PairSpec {
  std::string target, reference, output;
  double target_age = 0, ref_age = 0;
  std::vector<std::string> target_masks, ref_masks;  // one fasta per chromosome, or none
  std::string coal;                                   // --pairs `coal=FILE`: the pair's epochs and starting rates ("": --bins)
  std::string cond;                                   // `--mode count_topo`: the conditioning sample's file ("": every other mode)
  size_t line = 0;                                    // --pairs: the line of the list (1-based), and how many ages it carried
  int ages_given = 0;
  std::string target_name, ref_name;                  // --samples: the NAMEs of the two lines
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

}  // namespace colate_drv
