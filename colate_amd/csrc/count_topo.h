// colate_amd/csrc/count_topo.h -- `Colate --mode count_topo` (internal to libcolate_amd.so): what the cursor walk, the host twin
// of the indexed form (count_topo.cpp) and the device stage (count_topo_kernel.hip) share.
//
// THE CONTRACT (include/coal/coal.cpp:4523-4781, restated).  For a conditioning sample C (--input), a target T and a reference R
// the mode walks the .mut rows; at every SNP where C carries the derived allele and T and R both have data it samples one allele
// from T and one from R and prints the SNP with +1 where T is derived and R ancestral, with -1 for the converse.
// Rows.  Per chromosome the rows of <mut>_chr<name>.mut[.gz] (without --chr: <mut> itself, the empty name).  A row is SEARCHED
//   when flipped == 0, it has one branch, the float age_begin <= age_end (`<=`: rows with equal ages are searched here and not in
//   `--mode compare_tmp` or `--mode mut`), and both alleles are one of A C G T (or 0 / 1).
// Cursors.  At every searched row each of the three cursors advances while it is in the chromosome and bp < pos; none depends on
//   another.  The counts are NOT reset in front of a search (compare_tmp resets them), so whether the cursor moved does not matter:
//   T (and likewise R) HITS a row iff its cursor stands on a record of the row's chromosome, position and alleles with AAF + DAF > 0.
//   Over a file's walk index (mut_pairs.cpp: build_walk_index) that is (idx.DAF | idx.AAF) != 0 and nothing else.
//   C is never checked against the row: the reference uses DAF_cond and AAF_cond of whatever record C's cursor stands on -- the
//   first record of the chromosome at or behind the row; behind the chromosome's last record the record that follows the
//   chromosome's run in the file, or the file's last record where the reads have run out.  C QUALIFIES a row iff that record has
//   DAF > 0 and DAF + AAF > 0.  The COND INDEX of a file holds those counts row by row (mut_pairs.cpp: build_row_index).
// Draws.  A row QUALIFIES for the triple iff T hits, R hits and C qualifies.  At every qualifying row, and only there, two uniforms
//   are drawn from the run's std::mt19937 (seeded once per run) through uniform_real_distribution<double>(0, 1), each ROUNDED TO
//   FLOAT: qualifying row number k of the run, counted across chromosomes, uses uniforms 2k and 2k + 1 of the seed's stream.  With
//   pT = (double)DAF_T / N_T and pR likewise, the floats promoted back to double: +1 when d1 <= pT && d2 > pR, -1 when d1 > pT &&
//   d2 <= pR, else nothing is printed.  (A uniform just below 1 rounds up to 1.0f, and 1.0f <= 1.0 holds.)
// Output.  One line per printed row, `name pos age_begin age_end sign value` with value = sign * (double)DAF_C / N_C; the ages are
//   floats in the stream's default format.  No windows, no totals.
// The run's first chromosome.  The three name buffers are uninitialised in the reference (coal.cpp:4585).  In its compiled form
//   (oracle/_ref/Colate_ref) they do not hold the listed name, so each skip loop reads one record before it compares -- what
//   compare_tmp.h records as "a fresh cursor matches no name" -- and the cursor walk below does the same.  In this mode it changes
//   no output: nothing is reset, every cursor then advances to the row's lower bound whichever record it started from, and with the
//   empty name of a run without --chr a file whose first record carries another name leaves T and R without a hit either way.  The
//   `nochr` fixture is the reference's file for such a run.
//
// THE INDEXED FORM.  Per sample two bit planes over the searched rows, `hit` from its walk index and `qualifies` from its cond
// index, each chromosome starting on a 64-bit word (mask_words, interval_walk.h).  Per triple Q = hitT & hitR & qualC; the rank of
// a set bit of Q among the triple's set bits, chromosomes in order, is the row's position in the stream; two bit planes come out,
// `plus` and `minus`, and the number of qualifying rows.  Integers decide everything but the two double quotients and the two
// float roundings of draw_sign, which depend on one row alone: no result depends on an order of operations, and there are no
// atomics of any kind.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "colate_amd.h"
#include "interval_walk.h"

namespace colate_topo {

using colate_iw::block_of_pos;
using colate_iw::Idx;
using colate_iw::Row;
using Triple = colate_topo_triple;
static_assert(sizeof(Triple) == 12, "topo triple");

constexpr int kPlaneTile = 256;             // threads of a plane workgroup: four words of one array
constexpr int kDrawWaves = 4;               // waves of a draw workgroup: each takes every fourth tile of its chromosome
constexpr int kTileWords = 64;              // words a wave scans at once, one per lane
constexpr int kTileRows = kTileWords * 64;  // colate_topo_samples_tile()

COLATE_IC_HD inline bool hits(const Idx& x) { return (x.DAF | x.AAF) != 0; }
COLATE_IC_HD inline bool qualifies(const Idx& c) { return c.DAF > 0; }
// +1, -1 or 0 at a qualifying row from the two uniforms of its rank (coal.cpp:4742-4749)
COLATE_IC_HD inline int draw_sign(const Idx& t, const Idx& r, double u1, double u2) {
  const float d1 = (float)u1, d2 = (float)u2;
  const int N_target = (int)t.DAF + (int)t.AAF, N_ref = (int)r.DAF + (int)r.AAF;
  const double pT = (double)t.DAF / N_target, pR = (double)r.DAF / N_ref;
  if ((double)d1 <= pT && (double)d2 > pR) return 1;
  if ((double)d1 > pT && (double)d2 <= pR) return -1;
  return 0;
}

// THE AGE PROFILE (colate_topo_profile).  The epoch of a searched row, for epochs[E] finite and strictly ascending, 1 <= E <=
// kMaxProfileEpochs: mid = 0.5f * (age_begin + age_end) in single precision -- one float addition, rounded; the product is exact --
// and the number of e in 1 .. E - 1 with epochs[e] <= (double)mid.  Total: a NaN or negative mid gives 0, +inf gives E - 1.  Per
// (triple, epoch) three integers: the rows of the epoch set in the `plus` plane, in the `minus` plane, and in Q.  Integers only:
// no result depends on an order of operations, and no floating-point sum is formed anywhere.
constexpr int kMaxProfileEpochs = 1024;
COLATE_IC_HD inline int age_epoch(float age_begin, float age_end, const double* epochs, int E) {
  const float mid = 0.5f * (age_begin + age_end);
  int lo = 0, hi = E - 1;  // the answer lies in [lo, hi]: at most 10 steps
  while (lo < hi) {
    const int m = (lo + hi + 1) >> 1;
    if (epochs[m] <= (double)mid) lo = m;
    else hi = m - 1;
  }
  return lo;
}

// THE BLOCKS OF THIS MODE (colate_topo_blocks, colate_topo_profile_blocks, `--jackknife`).  A function of the searched rows alone,
// not of the triple: with nbpb bases per block the block of a searched row within its chromosome is k(pos) = block_of_pos(pos,
// nbpb) (interval_walk.h: pos in (k nbpb, (k + 1) nbpb], everything up to nbpb in block 0).  A chromosome owns k(pos of its last
// searched row) + 1 blocks -- the largest k of its rows; positions ascend in every indexed form -- or 1 block without a searched
// row; a row's global block is the sum of the earlier chromosomes' block counts plus k(pos); nb is the sum over the chromosomes.  A
// block that holds no searched row exists and is all zeros (a gap in the positions leaves one).  These are NOT the blocks of
// `--mode mut`, which start at a pair's first used row and so depend on the pair.
// Per (triple, block, epoch) the three integers of the age profile, from the same draws: a triple's qualifying row number k,
// counted across the whole genome in order, reads uniforms 2k and 2k + 1 whatever the blocks, so the sum over a triple's blocks is
// colate_topo_profile's counts in every integer, for every nbpb.
constexpr int kMaxTopoBlocks = 65535;
constexpr long long kMaxBlockPartialBytes = 1LL << 30;  // one triple's partials, 12 E nb bytes
// blk_off[C + 1] from max_pos[C], the largest position of each chromosome's searched rows (0 without one).  Refused: nbpb < 1, a
// position at or above 2^31 - nbpb, more than kMaxTopoBlocks blocks (COLATE_ELIMIT with the needed number).
int block_offsets(int C, const int* max_pos, int nbpb, int* blk_off);

// THE BLOCK JACKKNIFE (colate_topo_jackknife): the one copy of the arithmetic, host only.  counts[nb][E][3] of one triple; cell e <
// E is epoch e, cell E the sum over the epochs.  Per cell, with a_j = plus, b_j = minus, n_j = a_j + b_j of block j, the used blocks
// those with n_j > 0 in ascending order, g of them, and the integers A = sum a_j, M = sum b_j, n = A + M: D = (A - M) / n; for g >=
// 2 the weighted delete-one jackknife of Busing, Meijer and van der Leeden (1999) -- theta_j = ((A - a_j) - (M - b_j)) / (n - n_j),
// h_j = n / n_j, D_jack = g D - sum_j ((n - n_j) / n) theta_j, pseudo-values tau_j = h_j D - (h_j - 1) theta_j, se^2 = (1 / g) sum_j
// (tau_j - D_jack)^2 / (h_j - 1), Z = D_jack / se -- every operation an IEEE double, rounded, in the order written in
// count_topo.cpp, no contraction.  out[E + 1][4]: D, D_jack, se, Z, NaN for "not available" (all four at n == 0; all but D at
// g < 2; Z where se is not > 0); used[E + 1]: g.
void jackknife(int nb, int E, const long long* counts, double* out, int* used);

// THE EXPECTED COUNTS (colate_topo_expected_blocks, `--expected`): what the sampled counts estimate, formed directly.  Given the
// read counts a qualifying row prints +1 with probability pT (1 - pR) and -1 with probability (1 - pT) pR; summing those over the
// rows is the Rao-Blackwellised statistic -- the same expectation, a strictly smaller variance, no seed -- and where T and R are
// fixed at every row (DAF == 0 or AAF == 0) it IS the sampled count.  A row qualifies as above: hits(T) && hits(R) && qualifies(C).
// At a qualifying row, with N_T = DAF_T + AAF_T, N_R = DAF_R + AAF_R and every value an unsigned integer,
//   plus_fx  = floor((DAF_T * AAF_R) * 2^30 / (N_T * N_R)),   minus_fx = floor((AAF_T * DAF_R) * 2^30 / (N_T * N_R)):
// the two probabilities in units of 2^-30 (kExpectedOne), rounded down.  With the 16-bit counts of an Idx a numerator is below 2^32,
// a shifted one below 2^62, and every intermediate fits 64 bits.  plus_fx + minus_fx <= 2^30 per row; a row at which T and R are
// both fixed adds exactly 2^30 to plus iff T is all derived and R all ancestral, exactly 2^30 to minus for the converse, else 0.
// Per (triple, block, epoch) -- the blocks of this mode, age_epoch -- three integers: sum plus_fx, sum minus_fx, and the qualifying
// rows, which are column 2 of colate_topo_profile_blocks whatever the uniforms.  Only integers are summed: no result depends on an
// order of operations, on the chunking or on the block size, and counts at a finer block size, regrouped, are those at a coarser
// multiple.  Each addend is short of the exact product by less than 2^-30, so a cell of n rows is short by less than n 2^-30.  With
// fewer than 2^31 searched rows (kMaxExpectedRows; more are refused, COLATE_ELIMIT) every cell, every sum over blocks and the
// jackknife's n = A + M stay below 2^62.  Every formula of the jackknife is a ratio of counts: it takes these scaled integers as
// they are.
constexpr int kExpectedShift = 30;
constexpr long long kExpectedOne = 1LL << kExpectedShift;
constexpr long long kMaxExpectedRows = (1LL << 31) - 1;
// The two addends of a qualifying row from the counts of T and R (N_T, N_R > 0) -- the one copy: the host twin, the kernel and the
// cursor path.  Counts below 2^16, an Idx's, take 64-bit arithmetic; larger ones, which only the record cursors of the host meet
// (32-bit counts), a 128-bit intermediate.
struct Addends {
  unsigned long long plus, minus;
};
// floor(num 2^30 / den) for num <= den < 2^34.  The device has no 64-bit integer division and the compiler's expansion of one is
// some 250 instructions, so a double quotient makes the first guess -- both operands are exact doubles, the shifted numerator having
// at most 32 significant bits, and the guess lies within one of the floor -- and the exact integer remainder decides: the result is
// the floor for every input, whatever the rounding of the division.
COLATE_IC_HD inline unsigned long long expected_quotient(unsigned long long num, unsigned long long den) {
  const unsigned long long shifted = num << kExpectedShift;
  unsigned long long q = (unsigned long long)((double)shifted / (double)den);
  long long r = (long long)(shifted - q * den);  // (|r| stays below 2^63: shifted < 2^62, and q den is within a few den of it)
  while (r < 0) q--, r += (long long)den;
  while (r >= (long long)den) q++, r -= (long long)den;
  return q;
}
COLATE_IC_HD inline Addends expected_addends(unsigned long long DAF_T, unsigned long long AAF_T, unsigned long long DAF_R, unsigned long long AAF_R) {
#ifndef __HIP_DEVICE_COMPILE__
  if ((DAF_T | AAF_T | DAF_R | AAF_R) >> 16) {
    const unsigned __int128 den = (unsigned __int128)(DAF_T + AAF_T) * (DAF_R + AAF_R);
    return Addends{(unsigned long long)((((unsigned __int128)DAF_T * AAF_R) << kExpectedShift) / den),
                   (unsigned long long)((((unsigned __int128)AAF_T * DAF_R) << kExpectedShift) / den)};
  }
#endif
  const unsigned long long den = (DAF_T + AAF_T) * (DAF_R + AAF_R);
  return Addends{expected_quotient(DAF_T * AAF_R, den), expected_quotient(AAF_T * DAF_R, den)};
}
COLATE_IC_HD inline Addends expected_addends(const Idx& t, const Idx& r) { return expected_addends(t.DAF, t.AAF, r.DAF, r.AAF); }

// The inputs of both stages: every row given is a searched row; idx[s * C + c] is sample s's walk index of chromosome c,
// cidx[s * C + c] its cond index.
struct View {
  int C = 0;
  const long long* row_off = nullptr;
  const Row* const* rows = nullptr;
  int S = 0;
  const Idx* const* idx = nullptr;
  const Idx* const* cidx = nullptr;
  int P = 0;
  const Triple* triples = nullptr;
  long long n_uniforms = 0;
  const double* uniforms = nullptr;
};
// What both calls refuse before anything is written (COLATE_EINVAL / COLATE_ELIMIT; colate_last_error() names it): NULLs, bad
// sizes, decreasing offsets, ids out of range, rows that descend, a negative stream length.
int check_view(const View& v);
int check_outputs(long long cap, const long long* word_off, const unsigned long long* plus, const unsigned long long* minus, const long long* draws);
int check_capacity(long long P, long long words, long long cap);
// the stream the triples need: 2 x the most qualifying rows of any (COLATE_ELIMIT with the needed length where it is longer than given)
int check_stream(const View& v, const long long* draws);
// The host twin / the device stage: word_off[C + 1], plus / minus [P][word_off[C]] with room for cap words each, draws[P].
int topo_view_host(const View& v, long long cap, long long* word_off, unsigned long long* plus, unsigned long long* minus, long long* draws);
int topo_view_device(const View& v, long long cap, long long* word_off, unsigned long long* plus, unsigned long long* minus, long long* draws);
// The age profile of the same draws, host twin / device stage: counts[P][E][3] -- plus, minus, qualifying per epoch (age_epoch) --
// and draws[P].  Refused besides what check_view and check_stream refuse, by name: E outside 1 .. kMaxProfileEpochs, an epoch that
// is not finite, neighbours that do not ascend, NULL outputs.  No plane leaves either form.
int check_epochs(int E, const double* epochs);
int topo_profile_host(const View& v, int E, const double* epochs, long long* counts, long long* draws);
int topo_profile_device(const View& v, int E, const double* epochs, long long* counts, long long* draws);
// The blocks of the view's rows (above): blk_off[C + 1].  No device.
int topo_blocks(int C, const long long* row_off, const Row* const* rows, int nbpb, int* blk_off);
// The age profile per block, host twin / device stage: counts[P][nb][E][3] and draws[P].  Refused besides what the profile refuses,
// by name and before anything is written: what topo_blocks refuses, an nb that is not blk_off[C], one triple's partials above
// kMaxBlockPartialBytes (COLATE_ELIMIT).
int check_blocks(const View& v, int E, int nbpb, int nb, std::vector<int>& blk_off);
int topo_profile_blocks_host(const View& v, int E, const double* epochs, int nbpb, int nb, long long* counts, long long* draws);
int topo_profile_blocks_device(const View& v, int E, const double* epochs, int nbpb, int nb, long long* counts, long long* draws);
// A block as the device stage takes it: the rows [first, end) of chromosome c (first == end: no row)
struct Segment {
  int c, first, end;
};
// seg[nb] of the view's blocks: every searched row lies in exactly one
void block_segments(const View& v, int nbpb, const int* blk_off, Segment* seg);
// The expected counts per block, host twin / device stage: counts[P][nb][E][3] -- sum plus_fx, sum minus_fx, qualifying rows.  No
// stream goes in (v.n_uniforms and v.uniforms are not read) and no draws come out.  Refused, by name and before anything is
// written: what the profile per block refuses of the same arguments, and kMaxExpectedRows.
int check_expected(const View& v, int E, const double* epochs, int nbpb, int nb, const long long* counts, std::vector<int>& blk_off);
int topo_expected_blocks_host(const View& v, int E, const double* epochs, int nbpb, int nb, long long* counts);
int topo_expected_blocks_device(const View& v, int E, const double* epochs, int nbpb, int nb, long long* counts);

// THE CURSOR WALK of one chromosome: the reference's loop over three record cursors, correct for every input.  Cur: a cursor
// with match, bp, anc, der, AAF, DAF, set_name() and next() (mut_pairs.cpp: Cursor); RowT: pos, anc, der.  draw(): the next
// uniform of the run's stream; emit(i, sign, DAF_cond, N_cond): row i prints.  fresh: the run's first chromosome (above).
// drew(i): row i qualifies, printed or not (the age profile counts those rows; nothing by default).
struct NoRowSink {
  void operator()(size_t) const {}
};
template <class Cur, class RowT, class Draw, class Emit, class Drew = NoRowSink>
void cursor_walk_chromosome(Cur& cnd, Cur& tgt, Cur& ref, const char* name, bool fresh, const RowT* rows, size_t n, Draw&& draw, Emit&& emit,
                            Drew&& drew = Drew()) {
  Cur* const cur[3] = {&cnd, &tgt, &ref};
  for (Cur* c : cur) {  // skip to this chromosome, coal.cpp:4621-4652
    c->set_name(name);
    for (bool first = fresh; first || !c->match; first = false)
      if (!c->next()) break;
  }
  for (size_t i = 0; i < n; i++) {
    const RowT& m = rows[i];
    for (Cur* c : cur)
      while (c->match && c->bp < m.pos)
        if (!c->next()) break;
    const int N_cond = (int)((unsigned)cnd.DAF + (unsigned)cnd.AAF), N_target = (int)((unsigned)tgt.DAF + (unsigned)tgt.AAF),
              N_ref = (int)((unsigned)ref.DAF + (unsigned)ref.AAF);
    if (!tgt.match || tgt.bp != m.pos || tgt.anc != m.anc || tgt.der != m.der) continue;
    if (!ref.match || ref.bp != m.pos || ref.anc != m.anc || ref.der != m.der) continue;
    if (!(N_cond > 0 && N_ref > 0 && N_target > 0)) continue;
    if (!(cnd.DAF > 0)) continue;
    drew(i);
    const float d1 = (float)draw(), d2 = (float)draw();
    const double pT = (double)tgt.DAF / N_target, pR = (double)ref.DAF / N_ref;
    if ((double)d1 <= pT && (double)d2 > pR) emit(i, 1, cnd.DAF, N_cond);
    else if ((double)d1 > pT && (double)d2 <= pR) emit(i, -1, cnd.DAF, N_cond);
  }
}

}  // namespace colate_topo
