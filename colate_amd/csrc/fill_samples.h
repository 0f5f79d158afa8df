// colate_amd/csrc/fill_samples.h -- the table fill of `Colate --mode mut` for every pair of a sample list, over per-sample walk
// indices (internal to libcolate_amd.so): what the host side (fill_samples.cpp: the host twin, and fill_sample_pairs, which the
// command line of --samples fills its pairs through) and the device form (fill_samples_kernel.hip) share.
//
// THE CONTRACT is coal.cpp:2221-2297 as Engine::use_snp and Engine::sample restate it (mut_pairs.cpp), with age = ref_age = 0
// inside the fill (coal.cpp:2074-2075).  Per pair: the walk of interval_walk.h picks the used rows and their genome blocks; a
// used row is one FillRec (make_fill_rec); the pair owns a std::mt19937 on the run's seed and draws
// uniform_real_distribution<double>(0, 1) from it, record after record:
//   * begin <= 0 (the F path): row 0 of the A x A tables gets the un-divided weights at bin(age_end) (nothing for a bin >= A);
//     then 100 draws, x = u * (end - begin) + begin by a separate multiply and add, clamped at 0, each adding w_ns to the
//     not-shared table at bin(x) (nothing for a bin >= A);
//   * else 100 accepted draws, each adding w_sh and w_ns at bin(x); a draw with x < 0 or bin(x) >= A is drawn again.
// bin = age_bin_index(x, 10) (age_bins.hpp).  Tables per block in the order of Block::t: shared, not shared, shared row 0,
// not-shared row 0, [A] each, every sum from 0.0 in the order of the draws, every addition rounded.
// A used row that is never redrawn takes exactly 100 uniforms, so record number k of a pair reads the seed's stream at 100 k:
// that is what the device form relies on, and a pair in which it does not hold is handed back to the twin.
#pragma once
#include <cstdint>
#include <utility>
#include <vector>

#include "interval_walk.h"

namespace colate_drv {
class FastBin;  // age_bins.hpp
}

namespace colate_fs {

constexpr int kDraws = 100;  // coal.cpp:2073 num_samples

// Per pair p: nb, used, the tables [nb[p]][4][A] at tables[table_off[p]], the 32-bit words its generator has given out at the
// end of the fill (a std::mt19937 on the seed, discard(words[p]), is the run's generator there), and the two flags.
struct Result {
  std::vector<int> nb, handed_back, near_band;
  std::vector<long long> used;
  std::vector<size_t> table_off;  // [P + 1], in doubles
  std::vector<double> tables;
  std::vector<unsigned long long> words;
  int chunks = 0;          // device form: chunks of the write pass
  double kernel_s = 0.0;   // device form: seconds between the events around its kernels
};

// what both forms refuse: check_view, and A other than the 185 bins of colate_age_grid (COLATE_EINVAL)
int check_fill(const colate_iw::View& v, int A);
// nb, used, table_off and the zeroed tables of `out` from the counts [P][C] of a walk
int size_result(const colate_iw::View& v, int A, const int* cnt, const int* last, std::vector<int>& blk0, Result& out);
// The twin's fill of pair p (blk0: the pair's [C]): tables (zeroed here), words and near_band of `out` at p.  bands: the guard
// bands near_band is measured against (null: only the redraw conditions count).
void twin_pair(const colate_iw::View& v, int p, int A, unsigned seed, const int* blk0, const colate_drv::FastBin* bands, Result& out);
// runs of consecutive pairs whose records fit `budget_recs`; a larger pair goes alone
std::vector<std::pair<int, int>> plan_chunks(int P, const long long* rec_off, long long budget_recs);

int fill_view_host(const colate_iw::View& v, int A, unsigned seed, Result& out);
int fill_view_device(const colate_iw::View& v, int A, unsigned seed, Result& out);

}  // namespace colate_fs
