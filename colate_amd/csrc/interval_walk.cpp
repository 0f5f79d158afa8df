// colate_amd/csrc/interval_walk.cpp -- the host side of colate_interval_walk and colate_interval_fit_samples
// (interval_walk.h: the walk contract): the argument checks both forms run before anything is staged, the host twin of
// the two device passes -- a plain loop over the arrays, not a call into the table-fill engine, so that the two can be
// compared --, and the C entry points, which view the caller's back-to-back arrays chromosome by chromosome.
#include <algorithm>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "colate_amd.h"
#include "colate_internal.h"
#include "interval_groups.h"
#include "interval_walk.h"

using colate::fail;

namespace colate_iw {

long long mask_words(int C, const long long* row_off, long long* word_off) {
  long long w = 0;
  for (int c = 0; c < C; c++) {
    if (word_off) word_off[c] = w;
    w += (row_off[c + 1] - row_off[c] + 63) / 64;
  }
  if (word_off) word_off[C] = w;
  return w;
}

int check_view(const View& v) {
  if (v.C < 1 || v.S < 1 || v.P < 1 || v.M < 0)
    return fail(COLATE_EINVAL, "bad sizes C=%d S=%d M=%d P=%d (at least one chromosome, one sample and one pair)", v.C, v.S, v.M, v.P);
  if (!v.row_off) return fail(COLATE_EINVAL, "NULL pointer argument");
  if (v.nbpb < 1) return fail(COLATE_EINVAL, "num_bases_per_block = %d must be at least 1", v.nbpb);
  if (v.row_off[0] != 0) return fail(COLATE_EINVAL, "row_off[0] = %lld must be 0", v.row_off[0]);
  for (int c = 0; c < v.C; c++) {
    if (v.row_off[c + 1] < v.row_off[c])
      return fail(COLATE_EINVAL, "row_off decreases at chromosome %d (%lld after %lld)", c, v.row_off[c + 1], v.row_off[c]);
    if (v.row_off[c + 1] - v.row_off[c] > 0x7fffffffLL) return fail(COLATE_ELIMIT, "chromosome %d has 2^31 rows or more", c);
  }
  if (!v.rows || !v.idx || !v.pairs || (v.M > 0 && !v.masks)) return fail(COLATE_EINVAL, "NULL pointer argument");
  const long long n = v.row_off[v.C];
  for (int c = 0; c < v.C; c++)
    if (v.row_off[c + 1] > v.row_off[c] && !v.rows[c]) return fail(COLATE_EINVAL, "NULL pointer argument");
  for (size_t k = 0; n > 0 && k < (size_t)v.S * v.C; k++)
    if (v.row_off[k % v.C + 1] > v.row_off[k % v.C] && !v.idx[k]) return fail(COLATE_EINVAL, "NULL pointer argument");
  for (size_t k = 0; n > 0 && k < (size_t)v.M * v.C; k++)
    if (v.row_off[k % v.C + 1] > v.row_off[k % v.C] && !v.masks[k]) return fail(COLATE_EINVAL, "NULL pointer argument");
  for (int p = 0; p < v.P; p++) {
    const Pair& pr = v.pairs[p];
    if (pr.target < 0 || pr.target >= v.S || pr.reference < 0 || pr.reference >= v.S)
      return fail(COLATE_EINVAL, "pair %d: sample id out of range (target %d, reference %d, %d samples)", p, pr.target, pr.reference, v.S);
    if (pr.target_mask < -1 || pr.target_mask >= v.M || pr.reference_mask < -1 || pr.reference_mask >= v.M)
      return fail(COLATE_EINVAL, "pair %d: mask id out of range (target mask %d, reference mask %d, %d masks; -1: none)", p,
                  pr.target_mask, pr.reference_mask, v.M);
  }
  const long long pos_limit = 0x80000000LL - v.nbpb;
  for (int c = 0; c < v.C; c++) {
    const long long nc = v.row_off[c + 1] - v.row_off[c];
    for (long long i = 0; i < nc; i++) {
      const int pos = v.rows[c][i].pos;
      if (pos >= pos_limit)
        return fail(COLATE_EINVAL, "chromosome %d, row %lld: position %d at or above 2^31 - num_bases_per_block", c, i, pos);
      if (pos < 0 || (i > 0 && pos < v.rows[c][i - 1].pos))
        return fail(COLATE_EINVAL, "chromosome %d, row %lld: position %d is negative or below the row in front (the walk index is one of ascending rows)", c, i, pos);
    }
  }
  return COLATE_OK;
}

namespace {

// One pair and chromosome, row by row: sink(i, t, r) for every used row.
template <class Sink>
void walk_chromosome(const View& v, int p, int c, Sink&& sink) {
  const Pair& pr = v.pairs[p];
  const long long n = v.row_off[c + 1] - v.row_off[c];
  const Row* const rows = v.rows[c];
  const Idx* const TI = v.idx[(size_t)pr.target * v.C + c];
  const Idx* const RI = v.idx[(size_t)pr.reference * v.C + c];
  const unsigned long long* const tm = pr.target_mask < 0 ? nullptr : v.masks[(size_t)pr.target_mask * v.C + c];
  const unsigned long long* const rm = pr.reference_mask < 0 ? nullptr : v.masks[(size_t)pr.reference_mask * v.C + c];
  auto pos = [rows](long long i) { return i < 0 ? -1 : rows[i].pos; };
  long long searched = -1, ref_pass = -1;
  for (long long i = 0; i < n; i++) {
    if (tm && !((tm[i >> 6] >> (i & 63)) & 1ull)) continue;
    if (rm && !((rm[i >> 6] >> (i & 63)) & 1ull)) continue;
    const Idx r = RI[i];
    const long long ref_from = searched;
    searched = i;
    if (r.DAF == 0 || r.prev_bp < pos(ref_from)) continue;
    const Idx t = TI[i];
    const long long tgt_from = ref_pass;
    ref_pass = i;
    if ((t.DAF | t.AAF) == 0 || t.prev_bp < pos(tgt_from)) continue;
    sink(i, t, r);
  }
}

}  // namespace

void host_count(const View& v, int p, int* cnt, int* last_block) {
  for (int c = 0; c < v.C; c++) {
    int n = 0;
    long long last = -1;
    walk_chromosome(v, p, c, [&](long long i, const Idx&, const Idx&) { n++, last = i; });
    cnt[c] = n;
    last_block[c] = last < 0 ? -1 : block_of_pos(v.rows[c][last].pos, v.nbpb);
  }
}

void offsets_from_counts(int P, int C, const int* cnt, const int* last_block, int* blk0, long long* nb, long long* rec_off) {
  rec_off[0] = 0;
  for (int p = 0; p < P; p++) {
    long long blocks = 0, recs = 0;
    for (int c = 0; c < C; c++) {
      const size_t k = (size_t)p * C + c;
      blk0[k] = (int)std::min<long long>(blocks, 0x7fffffffLL);
      blocks += (long long)last_block[k] + 1 > 0 ? (long long)last_block[k] + 1 : 1;
      recs += cnt[k];
    }
    nb[p] = blocks;
    rec_off[p + 1] = rec_off[p] + recs;
  }
}

void host_write(const View& v, int p, const int* blk0, colate_ic::IntervalRec* recs, int* block) {
  long long at = 0;
  for (int c = 0; c < v.C; c++)
    walk_chromosome(v, p, c, [&](long long i, const Idx& t, const Idx& r) {
      const Row& m = v.rows[c][i];
      recs[at] = make_rec(m, t, r);
      block[at] = blk0[c] + block_of_pos(m.pos, v.nbpb);
      at++;
    });
}

void host_write_fill(const View& v, int p, const int* blk0, colate_drv::FillRec* recs, FillSide* side, int* block) {
  long long at = 0;
  for (int c = 0; c < v.C; c++)
    walk_chromosome(v, p, c, [&](long long i, const Idx& t, const Idx& r) {
      const Row& m = v.rows[c][i];
      recs[at] = make_fill_rec(m, t, r, side[at]);
      block[at] = blk0[c] + block_of_pos(m.pos, v.nbpb);
      at++;
    });
}

int finish_counts(int P, int C, const int* cnt, const int* last_block, int* blk0, int* nb, long long* rec_off) {
  std::vector<long long> nb64((size_t)P);
  offsets_from_counts(P, C, cnt, last_block, blk0, nb64.data(), rec_off);
  for (int p = 0; p < P; p++) {
    if (nb64[(size_t)p] > 0x7fffffffLL) return fail(COLATE_ELIMIT, "pair %d: %lld genome blocks", p, nb64[(size_t)p]);
    nb[p] = (int)nb64[(size_t)p];
  }
  return COLATE_OK;
}

int check_walk_outputs(long long cap, const long long* rec_off, const int* nb, const colate_ic::IntervalRec* recs, const int* block) {
  if (!rec_off || !nb) return fail(COLATE_EINVAL, "NULL pointer argument");
  if (cap < 0) return fail(COLATE_EINVAL, "cap = %lld is negative", cap);
  if (cap > 0 && (!recs || !block)) return fail(COLATE_EINVAL, "NULL pointer argument");
  return COLATE_OK;
}

int check_capacity(long long total, long long cap) {
  if (total > cap) return fail(COLATE_ELIMIT, "the pairs use %lld records, room for %lld (needed: %lld)", total, cap, total);
  return COLATE_OK;
}

int walk_view_host(const View& v, long long cap, long long* rec_off, int* nb, colate_ic::IntervalRec* recs, int* block) {
  if (int rc = check_walk_outputs(cap, rec_off, nb, recs, block)) return rc;
  if (int rc = check_view(v)) return rc;
  const size_t PC = (size_t)v.P * v.C;
  std::vector<int> cnt(PC), last(PC), blk0(PC), nbs((size_t)v.P);
  std::vector<long long> off((size_t)v.P + 1);
  for (int p = 0; p < v.P; p++) host_count(v, p, cnt.data() + (size_t)p * v.C, last.data() + (size_t)p * v.C);
  if (int rc = finish_counts(v.P, v.C, cnt.data(), last.data(), blk0.data(), nbs.data(), off.data())) return rc;
  if (int rc = check_capacity(off[(size_t)v.P], cap)) return rc;
  for (int p = 0; p < v.P; p++) host_write(v, p, blk0.data() + (size_t)p * v.C, recs + off[(size_t)p], block + off[(size_t)p]);
  std::memcpy(rec_off, off.data(), sizeof(long long) * off.size()), std::memcpy(nb, nbs.data(), sizeof(int) * nbs.size());
  return COLATE_OK;
}

int check_fit_args(const View& v, const FitArgs& a) {
  if (a.B < 1 || a.E < 1) return fail(COLATE_EINVAL, "bad sizes B=%d E=%d (at least one replicate and one epoch)", a.B, a.E);
  if (a.E > 1024) return fail(COLATE_ELIMIT, "E=%d above the compiled limit (1024)", a.E);
  if (a.B > 65535) return fail(COLATE_ELIMIT, "B=%d above the grid of the grouped bootstrap kernel (65535)", a.B);
  if (!a.epochs || !a.init_rates || !a.out_nb || !a.out_used || !a.out_R || !a.out_dropped || !a.out_rates || !a.out_iters ||
      !a.out_loglik || !a.out_flags)
    return fail(COLATE_EINVAL, "NULL pointer argument");
  if (int rc = check_view(v)) return rc;
  if ((long long)v.P * a.B > 0x7fffffffLL) return fail(COLATE_ELIMIT, "P x B = %lld replicates", (long long)v.P * a.B);
  // epochs, starting rates and iteration limits, on one stand-in row at the first point of the age grid (a used SNP may
  // begin there) in one block of weight one
  double grid[COLATE_MAX_AGE_BINS];
  if (colate_age_grid(grid, COLATE_MAX_AGE_BINS) != colate_ic::kBins) return fail(COLATE_EINVAL, "the age grid has not %d points", colate_ic::kBins);
  const int kind0 = 0;
  const double one = 1.0, zero = 0.0;
  std::vector<double> bw((size_t)a.B, one);
  return colate::check_bootstrap_interval_batch(a.B, 1, 1, a.E, &kind0, &grid[0], &grid[0], bw.data(), &zero, a.epochs, a.init_rates,
                                                a.max_iter, a.min_iter, a.rel_tol, a.rate_floor, a.out_rates, a.out_iters, a.out_loglik,
                                                a.out_flags);
}

int draw_pair_weights(unsigned seed, int B, int P, const int* nb, std::vector<double>& weights) {
  size_t total = 0;
  for (int p = 0; p < P; p++) {
    if (nb[p] > COLATE_INTERVAL_MAX_BLOCKS)
      return fail(COLATE_ELIMIT, "pair %d: %d genome blocks above COLATE_INTERVAL_MAX_BLOCKS (%d)", p, nb[p], COLATE_INTERVAL_MAX_BLOCKS);
    total += (size_t)B * nb[p];
  }
  weights.resize(total);
  size_t at = 0;
  for (int p = 0; p < P; p++) {
    std::mt19937 rng(seed);  // (every pair from the run's seed, as its single run: coal.cpp:3350-3357)
    if (int rc = colate_bootstrap_weights(&rng, B, nb[p], weights.data() + at)) return rc;
    at += (size_t)B * nb[p];
  }
  return COLATE_OK;
}

int fit_samples_view_host(const View& v, const FitArgs& a, int math) {
  if (math != 0 && math != 1) return fail(COLATE_EINVAL, "math must be 0 (<cmath>) or 1 (em_math)");
  if (int rc = check_fit_args(v, a)) return rc;
  const size_t PC = (size_t)v.P * v.C;
  std::vector<int> cnt(PC), last(PC), blk0(PC), nb((size_t)v.P);
  std::vector<long long> off((size_t)v.P + 1);
  for (int p = 0; p < v.P; p++) host_count(v, p, cnt.data() + (size_t)p * v.C, last.data() + (size_t)p * v.C);
  if (int rc = finish_counts(v.P, v.C, cnt.data(), last.data(), blk0.data(), nb.data(), off.data())) return rc;
  std::vector<double> weights;
  if (int rc = draw_pair_weights(a.seed, a.B, v.P, nb.data(), weights)) return rc;
  std::vector<colate_ic::IntervalRec> recs((size_t)off[(size_t)v.P]);
  std::vector<int> block(recs.size());
  for (int p = 0; p < v.P; p++) host_write(v, p, blk0.data() + (size_t)p * v.C, recs.data() + off[(size_t)p], block.data() + off[(size_t)p]);
  const std::vector<double> ep = colate_ic::repeat_rows(a.epochs, a.E, v.P), init = colate_ic::repeat_rows(a.init_rates, a.E, v.P);
  if (int rc = colate_interval_fit_groups_host(v.P, a.B, a.E, off.data(), recs.data(), block.data(), nb.data(), weights.data(), ep.data(),
                                               init.data(), a.max_iter, a.min_iter, a.rel_tol, a.rate_floor, a.out_R, a.out_dropped,
                                               a.out_rates, a.out_iters, a.out_loglik, a.out_flags, math))
    return rc;
  for (int p = 0; p < v.P; p++) a.out_nb[p] = nb[(size_t)p], a.out_used[p] = off[(size_t)p + 1] - off[(size_t)p];
  return COLATE_OK;
}

namespace {

// the caller's back-to-back arrays, chromosome by chromosome (the pointers live in `store`)
struct FlatView {
  View v;
  std::vector<const Row*> rows;
  std::vector<const Idx*> idx;
  std::vector<const unsigned long long*> masks;
  FlatView(int C, const long long* row_off, const Row* r, int S, const Idx* x, int M, const unsigned long long* m, int P,
           const Pair* pairs, int nbpb) {
    v.C = C, v.row_off = row_off, v.S = S, v.M = M, v.P = P, v.pairs = pairs, v.nbpb = nbpb;
    bool ok = C >= 1 && S >= 1 && M >= 0 && row_off && row_off[0] == 0;
    for (int c = 0; ok && c < C; c++) ok = row_off[c + 1] >= row_off[c];
    if (!ok) {  // (check_view names what is wrong with the sizes or offsets: nothing below is dereferenced before it)
      static const Row* const no_rows = nullptr;
      static const Idx* const no_idx = nullptr;
      static const unsigned long long* const no_mask = nullptr;
      v.rows = r ? &no_rows : nullptr, v.idx = x ? &no_idx : nullptr, v.masks = m ? &no_mask : nullptr;
      return;
    }
    const long long n = row_off[C];
    std::vector<long long> woff((size_t)C + 1);
    const long long words = mask_words(C, row_off, woff.data());
    rows.resize((size_t)C), idx.resize((size_t)S * C), masks.resize((size_t)M * C);
    for (int c = 0; c < C; c++) rows[(size_t)c] = r ? r + row_off[c] : nullptr;
    for (int s = 0; s < S; s++)
      for (int c = 0; c < C; c++) idx[(size_t)s * C + c] = x ? x + (size_t)s * n + row_off[c] : nullptr;
    for (int k = 0; k < M; k++)
      for (int c = 0; c < C; c++) masks[(size_t)k * C + c] = m ? m + (size_t)k * words + woff[(size_t)c] : nullptr;
    v.rows = r ? rows.data() : nullptr, v.idx = x ? idx.data() : nullptr, v.masks = m ? masks.data() : nullptr;
  }
};

}  // namespace

}  // namespace colate_iw

using namespace colate_iw;

extern "C" {

int colate_interval_walk_tile(void) { return kTile; }

int colate_interval_walk_host(int C, const long long* row_off, const colate_walk_row* rows, int S, const colate_walk_idx* idx, int M,
                              const unsigned long long* masks, int P, const colate_walk_pair* pairs, int num_bases_per_block,
                              long long cap, long long* rec_off, int* nb, colate_interval_rec* recs, int* block) {
  const FlatView f(C, row_off, rows, S, idx, M, masks, P, pairs, num_bases_per_block);
  return walk_view_host(f.v, cap, rec_off, nb, recs, block);
}

int colate_interval_walk(int C, const long long* row_off, const colate_walk_row* rows, int S, const colate_walk_idx* idx, int M,
                         const unsigned long long* masks, int P, const colate_walk_pair* pairs, int num_bases_per_block, long long cap,
                         long long* rec_off, int* nb, colate_interval_rec* recs, int* block) {
  const FlatView f(C, row_off, rows, S, idx, M, masks, P, pairs, num_bases_per_block);
  return walk_view_device(f.v, cap, rec_off, nb, recs, block);
}

#define COLATE_FIT_ARGS                                                                                                              \
  FitArgs {                                                                                                                          \
    B, E, epochs, init_rates, seed, max_iter, min_iter, rel_tol, rate_floor, out_nb, out_used, out_R, out_dropped, out_rates, out_iters, \
        out_loglik, out_flags                                                                                                        \
  }

int colate_interval_fit_samples_host(int C, const long long* row_off, const colate_walk_row* rows, int S, const colate_walk_idx* idx,
                                     int M, const unsigned long long* masks, int P, const colate_walk_pair* pairs,
                                     int num_bases_per_block, int B, int E, const double* epochs, const double* init_rates,
                                     unsigned int seed, int max_iter, int min_iter, double rel_tol, double rate_floor, int* out_nb,
                                     long long* out_used, int* out_R, long long* out_dropped, double* out_rates, int* out_iters,
                                     double* out_loglik, int* out_flags, int math) {
  const FlatView f(C, row_off, rows, S, idx, M, masks, P, pairs, num_bases_per_block);
  return fit_samples_view_host(f.v, COLATE_FIT_ARGS, math);
}

int colate_interval_fit_samples(int C, const long long* row_off, const colate_walk_row* rows, int S, const colate_walk_idx* idx, int M,
                                const unsigned long long* masks, int P, const colate_walk_pair* pairs, int num_bases_per_block, int B,
                                int E, const double* epochs, const double* init_rates, unsigned int seed, int max_iter, int min_iter,
                                double rel_tol, double rate_floor, int* out_nb, long long* out_used, int* out_R, long long* out_dropped,
                                double* out_rates, int* out_iters, double* out_loglik, int* out_flags) {
  const FlatView f(C, row_off, rows, S, idx, M, masks, P, pairs, num_bases_per_block);
  return fit_samples_view_device(f.v, COLATE_FIT_ARGS);
}

}  // extern "C"
