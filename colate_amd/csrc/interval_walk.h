// colate_amd/csrc/interval_walk.h -- the pair walk of `--mode mut_interval` over per-sample walk indices (internal to
// libcolate_amd.so): what the device stage (interval_walk_kernel.hip) and its host twin (interval_walk.cpp) share.
//
// THE WALK CONTRACT (Engine::walk_indexed and the `cells` branch of Engine::use_snp, mut_pairs.cpp, operand for operand).
// Per pair and chromosome, rows i = 0 .. n - 1 in order, two states `searched` and `ref_pass`, both -1 at the
// chromosome's start; pos(-1) = -1:
//   * a row the pair's masks remove (the bit of row i is clear in the target's or in the reference's mask) changes nothing;
//   * otherwise ref_from = searched, searched = i; with r = RI[i]: r.DAF == 0 or r.prev_bp < pos(ref_from) skips the row;
//   * otherwise tgt_from = ref_pass, ref_pass = i; with t = TI[i]: (t.DAF | t.AAF) == 0 or t.prev_bp < pos(tgt_from) skips;
//   * otherwise the row is used and becomes one record (make_rec below: three separate roundings per weight).
// Blocks: within a chromosome the block of a used row is k(pos) = the steps of `while (base + nbpb < pos) base += nbpb`
// from base = 0 (block_of_pos); a chromosome contributes k(pos of its last used row) + 1 blocks, or 1 without a used row;
// a record's block is the sum of the earlier chromosomes' counts plus k(pos); nb is the sum over all chromosomes.
// Records are ordered by chromosome, then row.
//
// Integers decide everything but the record's four numbers, and those are a function of one row alone: nothing here
// depends on an order of floating-point operations, and there are no atomics of any kind.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "colate_amd.h"
#include "fill_device.h"
#include "interval_cells.h"

namespace colate_iw {

using Row = colate_walk_row;    // {int pos; float age_begin, age_end}: 12 bytes per .mut row a walk looks at
using Idx = colate_walk_idx;    // {int prev_bp; unsigned short DAF, AAF}: 8 bytes per row and sample (TmpFile::RowIdx)
using Pair = colate_walk_pair;  // {target, reference, target_mask, reference_mask}: sample ids, mask ids or -1
static_assert(sizeof(Row) == 12 && sizeof(Idx) == 8 && sizeof(Pair) == 16, "walk inputs");

constexpr int kTile = 256;  // rows of a chromosome one workgroup looks at per step: one row per thread
constexpr int kWaves = kTile / 64;

COLATE_IC_HD inline int block_of_pos(int pos, int nbpb) { return pos > 0 ? (pos - 1) / nbpb : 0; }

// What both records of a used row start from (use_snp): the target genotype rounded to a haploid call in single precision, and
// its two float products with the reference's derived count.
struct GenotypeProducts {
  float p_sh, p_ns;  // (derived, ancestral) of the target times DAF_ref
};
COLATE_IC_HD inline GenotypeProducts genotype_products(const Idx& t, const Idx& r) {
  const int tgt_DAF = t.DAF, tgt_AAF = t.AAF, DAF_ref = r.DAF;
  const int N_target = tgt_DAF + tgt_AAF;
  float f_DAF_target = (float)tgt_DAF, f_AAF_target = (float)tgt_AAF;
  f_DAF_target = (float)((double)f_DAF_target / (N_target / 2.0));
  f_AAF_target = (float)((double)f_AAF_target / (N_target / 2.0));
  f_DAF_target = roundf(f_DAF_target);
  f_AAF_target = roundf(f_AAF_target);
  return GenotypeProducts{f_DAF_target * (float)DAF_ref, f_AAF_target * (float)DAF_ref};
}

// a used row as one interval-dated observation (use_snp: the float product, the conversion and the double division are
// three separate roundings; -ffp-contract=off on the host and on the device)
COLATE_IC_HD inline colate_ic::IntervalRec make_rec(const Row& m, const Idx& t, const Idx& r) {
  const int N_ref = (int)r.DAF + (int)r.AAF;
  double age_begin = m.age_begin;
  if (age_begin < 0.0) age_begin = 0.0;
  const GenotypeProducts g = genotype_products(t, r);
  return colate_ic::IntervalRec{(float)age_begin, m.age_end, (double)g.p_sh / (double)N_ref, (double)g.p_ns / (double)N_ref};
}

// The same used row as `--mode mut` samples it (Engine::use_snp, the table branch; coal.cpp:2221-2297 with age = ref_age = 0):
// the record of fill_sample_kernel -- a hundredth of the weights, w_sh = +0.0 on the F path (age_begin <= 0) -- and, in `side`,
// the un-divided pair that the F path adds to row 0 of the reference's A x A tables.  Every product, conversion and division is
// a rounding of its own, as there.
struct FillSide {
  double e_sh, e_ns;
};
static_assert(sizeof(FillSide) == 16, "FillSide");
COLATE_IC_HD inline colate_drv::FillRec make_fill_rec(const Row& m, const Idx& t, const Idx& r, FillSide& side) {
  const int N_ref = (int)r.DAF + (int)r.AAF;
  double age_begin = m.age_begin;
  if (age_begin < 0.0) age_begin = 0.0;
  const GenotypeProducts g = genotype_products(t, r);
  side.e_sh = (double)g.p_sh / (double)N_ref, side.e_ns = (double)g.p_ns / (double)N_ref;
  const double hundredth = (double)N_ref * 100.0;
  const double w_sh = age_begin <= 0.0 ? 0.0 : (double)g.p_sh / hundredth;
  return colate_drv::FillRec{(float)age_begin, m.age_end, w_sh, (double)g.p_ns / hundredth};
}

// The inputs as both stages read them: chromosome c's rows are rows[c][0 .. row_off[c + 1] - row_off[c]); sample s's index
// of it idx[s * C + c]; mask m's bits of it masks[m * C + c] (bit i & 63 of word i >> 6 is row i).  Host pointers for the
// host twin; the device stage holds the same arrays back to back (DeviceInputs).
struct View {
  int C = 0;
  const long long* row_off = nullptr;
  const Row* const* rows = nullptr;
  int S = 0;
  const Idx* const* idx = nullptr;
  int M = 0;
  const unsigned long long* const* masks = nullptr;
  int P = 0;
  const Pair* pairs = nullptr;
  int nbpb = 0;
};
// words of a mask over all chromosomes, each chromosome starting on a word; word_off[C + 1] where given
long long mask_words(int C, const long long* row_off, long long* word_off);

// What both calls refuse (COLATE_EINVAL / COLATE_ELIMIT; message in colate_last_error()): NULLs, sizes, decreasing
// offsets, ids out of range, num_bases_per_block < 1, a position at or above 2^31 - num_bases_per_block.
int check_view(const View& v);

// The host twin's count pass of pair p: per chromosome the used rows and the block of the last one (-1: none).
void host_count(const View& v, int p, int* cnt, int* last_block);
// From the counts of pairs [0, P), [P][C]: blk0[P][C], the pair-relative first block of every chromosome; nb[P]; and
// rec_off[P + 1] from rec_off[0] = 0.
void offsets_from_counts(int P, int C, const int* cnt, const int* last_block, int* blk0, long long* nb, long long* rec_off);
// ... with nb as the int the callers take (COLATE_ELIMIT at 2^31 blocks)
int finish_counts(int P, int C, const int* cnt, const int* last_block, int* blk0, int* nb, long long* rec_off);
// The host twin's write pass of pair p: its records and pair-relative blocks at recs / block (room for the pair's count).
void host_write(const View& v, int p, const int* blk0, colate_ic::IntervalRec* recs, int* block);
// ... with the records of the table fill (make_fill_rec): recs / side / block have room for the pair's count
void host_write_fill(const View& v, int p, const int* blk0, colate_drv::FillRec* recs, FillSide* side, int* block);

// colate_interval_walk[_host] on a view: rec_off[P + 1], nb[P], records and blocks back to back, room for cap records
// (COLATE_ELIMIT with the needed total in the message where they do not fit).
int check_walk_outputs(long long cap, const long long* rec_off, const int* nb, const colate_ic::IntervalRec* recs, const int* block);
int check_capacity(long long total, long long cap);
int walk_view_host(const View& v, long long cap, long long* rec_off, int* nb, colate_ic::IntervalRec* recs, int* block);
int walk_view_device(const View& v, long long cap, long long* rec_off, int* nb, colate_ic::IntervalRec* recs, int* block);

// colate_interval_fit_samples[_host] on a view (the command line hands over the files' indices where they lie)
struct FitArgs {
  int B, E;
  const double *epochs, *init_rates;  // [E], for all pairs
  unsigned seed;
  int max_iter, min_iter;
  double rel_tol, rate_floor;
  int* out_nb;          // [P]
  long long* out_used;  // [P]: records of the pair
  int* out_R;
  long long* out_dropped;
  double* out_rates;  // [P][B][E]
  int* out_iters;     // [P][B]
  double* out_loglik;
  int* out_flags;
};
// what both forms refuse before anything is walked: check_view, sizes and limits, and epochs, starting rates and
// iteration limits as colate_bootstrap_em_interval_batch refuses them.  The library forms the records itself (weights
// in [0, 2], blocks not decreasing), so no sum can overflow: at most 2 n per cell, times at most nb per replicate.
int check_fit_args(const View& v, const FitArgs& a);
// every pair's block weights [B][nb[p]], one after the other, each pair from a fresh std::mt19937 on `seed`
// (colate_bootstrap_weights); COLATE_ELIMIT where a pair has more than COLATE_INTERVAL_MAX_BLOCKS blocks
int draw_pair_weights(unsigned seed, int B, int P, const int* nb, std::vector<double>& weights);
int fit_samples_view_host(const View& v, const FitArgs& a, int math);
int fit_samples_view_device(const View& v, const FitArgs& a);

}  // namespace colate_iw

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
namespace colate_iw {
// The inputs resident on the device: rows[n], idx[S][n], masks[M][words], pairs[P]; row_off[C + 1], word_off[C + 1].
struct DeviceInputs {
  int C = 0, S = 0, M = 0, P = 0, nbpb = 0;
  long long n = 0, words = 0;
  const long long *row_off = nullptr, *word_off = nullptr;
  const Row* rows = nullptr;
  const Idx* idx = nullptr;
  const unsigned long long* masks = nullptr;
  const Pair* pairs = nullptr;
};
// Count pass for pairs [p0, p1): cnt / last_block[(p - p0) * C + c].  One workgroup per (pair, chromosome).
hipError_t count_launch(const DeviceInputs& in, int p0, int p1, int* cnt, int* last_block, hipStream_t stream);
// Write pass for pairs [p0, p1): rec0[(p - p0) * C + c] is where the chromosome's records start in recs (and block, which
// may be null), blk0 its pair-relative first block, seg0 the index of that block in `off` (null: no ranges wanted) --
// every workgroup writes off[] for the blocks its chromosome owns: the first record at or behind each; off_end /
// rec_end: the last entry of `off`, written by the last workgroup.
hipError_t write_launch(const DeviceInputs& in, int p0, int p1, const long long* rec0, const int* blk0, const int* seg0,
                        colate_ic::IntervalRec* recs, int* block, long long* off, long long off_end, long long rec_end,
                        hipStream_t stream);
// The same pass writing the records of the table fill and their side array (make_fill_rec); `off` as above.
hipError_t write_fill_launch(const DeviceInputs& in, int p0, int p1, const long long* rec0, const int* blk0, const int* seg0,
                             colate_drv::FillRec* recs, FillSide* side, long long* off, long long off_end, long long rec_end,
                             hipStream_t stream);
}  // namespace colate_iw
#endif
