// colate_amd/csrc/compare_tmp.h -- `Colate --mode compare_tmp` (internal to libcolate_amd.so): what the cursor walk, the host
// twin of the indexed form (compare_tmp.cpp) and the device stage (compare_kernel.hip) share.
//
// THE CONTRACT (include/coal/coal.cpp:4297-4521, restated).  For a pair of samples and every window of a chromosome the mode
// prints the SNPs at which both samples have data and how many of those the two disagree on.
// Rows.  Per chromosome the rows of <mut>_chr<name>.mut[.gz] (without --chr: <mut> itself, the empty name).  A row is SEARCHED
//   when flipped == 0, it has one branch, the float age_begin < age_end, and both alleles are one of A C G T (or 0 / 1): the
//   row filter of `--mode mut` without its age_end >= 0.
// Cursors.  At every searched row both files' cursors search, neither depending on the other.  The counts are reset to 0 in
//   front of each search, so a search counts only if the cursor MOVED in it and stopped on a record of the row's position and
//   alleles with AAF + DAF > 0.  Over a file's walk index (mut_pairs.cpp: build_walk_index): sample s HITS row i iff
//   (idx.DAF | idx.AAF) != 0 and idx.prev_bp >= pos(the searched row in front); pos(-1) = -1 at the start of every chromosome
//   (never the last row of the chromosome before).  Both cursors search at every searched row, so a hit is a property of the
//   sample and the row alone: the pair stage has no state.
// Statistic.  A row is COUNTED for a pair iff both samples hit it.  The reference "samples an allele" with
//   dist_unif(rng) < DAF / (AAF + DAF) in INTEGER division: the quotient is 1 when AAF == 0 and 0 otherwise, and a uniform in
//   [0, 1) is always below 1 and never below 0.  The draw decides nothing: the sampled allele is fixed = (AAF == 0), and
//   num_mismatch counts the counted rows with fixed_target != fixed_reference.  (Two uniforms per counted row are drawn and
//   thrown away: --seed has no effect.)
// Windows.  binsize = 10 000 000; current_bp starts at the position of the file's FIRST RAW row, searched or not; in front of
//   every raw row `while (pos > current_bp + binsize)` prints a line and steps on; one more line at the chromosome's end.  With
//   raw positions that do not descend chromosome c has W_c = w(last raw pos) + 1 windows, w(pos) = pos > first ? (pos - first - 1)
//   / binsize : 0 (window_of): a position exactly on first + k binsize belongs to window k - 1, and windows without a counted
//   row print `0 0`.  A line is `name current_bp num_mismatch num_snps`, the counts doubles in the stream's default format.
//
// THE INDEXED FORM.  Per sample two bit planes over the searched rows, `hit` and `fixed & hit`, each chromosome starting on a
// 64-bit word (mask_words, interval_walk.h); per pair and window two popcounts over the window's row range:
//   snps = popc(hitT & hitR), mismatch = popc(hitT & hitR & (fixT ^ fixR)).
// Integers only: no result depends on an order of operations, and there are no atomics of any kind.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "colate_amd.h"
#include "interval_walk.h"

namespace colate_cmp {

using colate_iw::Idx;
using colate_iw::Pair;
using colate_iw::Row;

constexpr int kBinSize = 10000000;  // coal.cpp:4365
constexpr int kPlaneTile = 256;     // threads of a plane workgroup: four words of one sample
constexpr int kPairWaves = 4;       // waves of a pair workgroup: each takes every fourth window of its chromosome

// the window of a position in a chromosome whose first raw row lies at `first`
COLATE_IC_HD inline long long window_of(long long pos, long long first, long long window) { return pos > first ? (pos - first - 1) / window : 0; }
// a sample's two predicates at a row; prev_pos: the position of the searched row in front (-1: the chromosome's first)
COLATE_IC_HD inline bool hits(const Idx& x, int prev_pos) { return (x.DAF | x.AAF) != 0 && x.prev_bp >= prev_pos; }
COLATE_IC_HD inline bool fixed(const Idx& x) { return x.AAF == 0; }
// the bits of word k (rows 64 k .. 64 k + 63) that lie in the row range [r0, r1), which touches the word
COLATE_IC_HD inline unsigned long long range_bits(long long k, long long r0, long long r1) {
  const long long lo = r0 - 64 * k, hi = r1 - 64 * k;  // (hi >= 1, lo <= 63)
  unsigned long long m = ~0ull;
  if (lo > 0) m &= ~0ull << lo;
  if (hi < 64) m &= ~0ull >> (64 - hi);
  return m;
}

// The inputs of both stages (the arrays of interval_walk.h's View, without masks): every row given is a searched row.
struct View {
  int C = 0;
  const long long* row_off = nullptr;
  const Row* const* rows = nullptr;
  int S = 0;
  const Idx* const* idx = nullptr;
  int P = 0;
  const Pair* pairs = nullptr;
  const int *first_pos = nullptr, *last_pos = nullptr;  // [C]: the file's first and last raw rows
  int window = 0;
};
// What both calls refuse before anything is written (COLATE_EINVAL / COLATE_ELIMIT; colate_last_error() names it): NULLs, bad
// sizes, decreasing offsets, ids out of range, mask ids other than -1, window < 1, rows that descend, first_pos above the
// first searched row's position or last_pos below the last one's, 2^31 windows or more.
int check_view(const View& v);
// win_off[C + 1] and, for chromosome c, the W_c + 1 row bounds of its windows at win_row[win_off[c] + c ...]: window w holds
// the rows [b[w], b[w + 1]) of the chromosome.  Computed once per call and shared by all pairs, on the host for both stages.
void window_rows(const View& v, std::vector<long long>& win_off, std::vector<int>& win_row);
// sample s's planes[2][words]: hit, fixed & hit
void host_planes(const View& v, int s, const long long* word_off, long long words, unsigned long long* planes);
// The host twin / the device stage: win_off[C + 1], mismatch / snps [P][win_off[C]], room for cap ints each (COLATE_ELIMIT with
// the needed number in the message).
int compare_view_host(const View& v, long long cap, long long* win_off, int* mismatch, int* snps);
int compare_view_device(const View& v, long long cap, long long* win_off, int* mismatch, int* snps);
int check_outputs(long long cap, const long long* win_off, const int* mismatch, const int* snps);
int check_capacity(long long P, long long windows, long long cap);

// THE CURSOR WALK of one chromosome: the reference's loop over two record cursors, correct for every input.  Cur: a cursor
// with match, bp, anc, der, AAF, DAF, set_name() and next() (mut_pairs.cpp: Cursor); RowT: pos, anc, der.  row_window[i]: the
// lines printed in front of searched row i (the state of current_bp, which the raw rows alone decide).
// fresh: the run's first chromosome.  The reference's two name buffers are uninitialised there (coal.cpp:4359); in its compiled
// form they do not hold the empty string, so the skip loop reads one record even for the empty chromosome name of a run without
// --chr, and a first row at that record's position finds the cursor already on it: no move, no hit.  A fresh cursor therefore
// matches no name.
template <class Cur, class RowT>
void cursor_walk_chromosome(Cur& tgt, Cur& ref, const char* name, bool fresh, const RowT* rows, size_t n, const int* row_window,
                            int* mismatch, int* snps) {
  tgt.set_name(name), ref.set_name(name);
  for (bool first = fresh; first || !tgt.match; first = false)  // skip to this chromosome, coal.cpp:4381-4401
    if (!tgt.next()) break;
  for (bool first = fresh; first || !ref.match; first = false)
    if (!ref.next()) break;
  for (size_t i = 0; i < n; i++) {
    const RowT& m = rows[i];
    tgt.AAF = 0, tgt.DAF = 0;
    while (tgt.match && tgt.bp < m.pos)
      if (!tgt.next()) break;
    const int N_target = tgt.DAF + tgt.AAF;
    ref.DAF = 0, ref.AAF = 0;
    while (ref.match && ref.bp < m.pos)
      if (!ref.next()) break;
    const int N_ref = ref.DAF + ref.AAF;
    if (!tgt.match || tgt.bp != m.pos || tgt.anc != m.anc || tgt.der != m.der) continue;
    if (!ref.match || ref.bp != m.pos || ref.anc != m.anc || ref.der != m.der) continue;
    if (!(N_ref > 0 && N_target > 0)) continue;
    // a uniform in [0, 1) is below the integer quotient iff the quotient is at least 1
    const int target_sampled = tgt.DAF / (tgt.AAF + tgt.DAF) >= 1, ref_sampled = ref.DAF / (ref.AAF + ref.DAF) >= 1;
    mismatch[row_window[i]] += target_sampled != ref_sampled;
    snps[row_window[i]]++;
  }
}

}  // namespace colate_cmp

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
namespace colate_cmp {
// planes[S][2][words] of the resident inputs: one lane per (sample, searched row)
hipError_t planes_launch(const colate_iw::DeviceInputs& in, unsigned long long* planes, hipStream_t stream);
// mismatch / snps [(p - p0)][total windows] for pairs [p0, p1): one workgroup per (pair, chromosome); win_off[C + 1] and
// win_row as window_rows gives them, on the device
hipError_t pairs_launch(const colate_iw::DeviceInputs& in, int p0, int p1, const unsigned long long* planes, const long long* win_off,
                        const int* win_row, int* mismatch, int* snps, hipStream_t stream);
}  // namespace colate_cmp
#endif
