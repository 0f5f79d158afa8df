// colate_amd/csrc/walk_inputs.h -- what mut_pairs.cpp gives the drivers besides the tables: the engine's walk of a pair as
// interval-dated records, the inputs of a list of pairs read, decoded and indexed once (WalkInputs and its loader), and the cursor
// walks of `--mode compare_tmp` and `--mode count_topo` over them.
#pragma once
#include <memory>
#include <string>
#include <vector>

#include "colate_amd.h"
#include "interval_walk.h"
#include "mut_inputs.h"

namespace colate_drv {

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
  // the indexed inputs as the pair walk takes them (interval_walk.h), genome blocks of nbpb bases
  colate_iw::View walk_view(int nbpb) const {
    colate_iw::View v;
    v.C = (int)row_ptrs.size(), v.row_off = row_off.data(), v.rows = row_ptrs.data(), v.S = S, v.idx = idx_ptrs.data(), v.M = M;
    v.masks = mask_ptrs.data(), v.P = (int)pairs.size(), v.pairs = pairs.data(), v.nbpb = nbpb;
    return v;
  }
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
  // `--jackknife`: nbpb > 0 and blk_off[C + 1] in (count_topo.h: the blocks of this mode), blocks[P][nb][E][3] out -- the same
  // three integers per genome block, whose sum over the blocks is `counts`
  int nbpb = 0;
  const int* blk_off = nullptr;
  std::vector<long long> blocks;
};
// blk_off[C + 1] of the loaded searched rows for the cursor walk, which takes rows in any order: a chromosome owns the largest k of
// its rows + 1 blocks.  The library's code (colate_last_error() names a refusal); COLATE_EINVAL without loaded inputs.
int topo_cursor_blocks(const WalkInputs& loaded, int nbpb, std::vector<int>& blk_off);
bool topo_cursor_triples(const WalkInputs& loaded, const std::vector<std::string>& names, const std::vector<PairSpec>& triples, unsigned seed,
                         std::vector<std::vector<TopoLine>>& lines, std::vector<long long>& draws, TopoProfile* profile = nullptr);
// `--expected` on the cursor path (count_topo.h: the expected counts): the same walk with a `drew` sink that forms the two
// fixed-point addends of every qualifying row from the counts its cursors stand on -- 32 bits each, a 128-bit intermediate -- and
// bins them by block and epoch; the walk's draws read a constant and nothing is emitted.  profile.E, epochs, nbpb > 0 and blk_off
// in; profile.blocks[P][nb][E][3] -- sum plus_fx, sum minus_fx, qualifying rows -- and their sums over the blocks, profile.counts, out.
bool topo_cursor_expected(const WalkInputs& loaded, const std::vector<std::string>& names, const std::vector<PairSpec>& triples, TopoProfile& profile);
// mut_pairs.cpp: the cursor walk of `--mode compare_tmp` (compare_tmp.h: cursor_walk_chromosome) for every pair of a list over inputs
// loaded with RowSet::compare_tmp: mismatch / snps [P][sum of compare[c].windows].  Right for every input; false without loaded inputs.
bool compare_cursor_pairs(const WalkInputs& loaded, const std::vector<std::string>& names, const std::vector<PairSpec>& pairs,
                          std::vector<int>& mismatch, std::vector<int>& snps);
// collect_interval_records_pairs on inputs loaded before (the path `--samples` takes where a file has no walk index)
bool collect_interval_records_loaded(const WalkInputs& loaded, const std::vector<std::string>& names, const std::vector<PairSpec>& pairs,
                                     std::vector<PairRecords>& out);

}  // namespace colate_drv
