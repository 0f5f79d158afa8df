// colate_amd/csrc/compare_tmp.cpp -- the host side of colate_compare_samples (compare_tmp.h: the contract): the checks both
// forms run before anything is written, the window row ranges both forms share, the host twin of the two device kernels -- bit
// planes per sample, popcounts per pair and window --, and the C entry points, which view the caller's back-to-back arrays
// chromosome by chromosome.
#include <cstring>
#include <vector>

#include "colate_amd.h"
#include "colate_internal.h"
#include "compare_tmp.h"

using colate::fail;

namespace colate_cmp {

int check_view(const View& v) {
  if (v.C < 1 || v.S < 1 || v.P < 1)
    return fail(COLATE_EINVAL, "bad sizes C=%d S=%d P=%d (at least one chromosome, one sample and one pair)", v.C, v.S, v.P);
  if (!v.row_off || !v.first_pos || !v.last_pos) return fail(COLATE_EINVAL, "NULL pointer argument");
  if (v.window < 1) return fail(COLATE_EINVAL, "window = %d must be at least 1", v.window);
  if (v.row_off[0] != 0) return fail(COLATE_EINVAL, "row_off[0] = %lld must be 0", v.row_off[0]);
  for (int c = 0; c < v.C; c++) {
    if (v.row_off[c + 1] < v.row_off[c])
      return fail(COLATE_EINVAL, "row_off decreases at chromosome %d (%lld after %lld)", c, v.row_off[c + 1], v.row_off[c]);
    if (v.row_off[c + 1] - v.row_off[c] > 0x7fffffffLL) return fail(COLATE_ELIMIT, "chromosome %d has 2^31 rows or more", c);
  }
  if (!v.rows || !v.idx || !v.pairs) return fail(COLATE_EINVAL, "NULL pointer argument");
  for (int c = 0; c < v.C; c++)
    if (v.row_off[c + 1] > v.row_off[c] && !v.rows[c]) return fail(COLATE_EINVAL, "NULL pointer argument");
  for (size_t k = 0; k < (size_t)v.S * v.C; k++)
    if (v.row_off[k % v.C + 1] > v.row_off[k % v.C] && !v.idx[k]) return fail(COLATE_EINVAL, "NULL pointer argument");
  for (int p = 0; p < v.P; p++) {
    const Pair& pr = v.pairs[p];
    if (pr.target < 0 || pr.target >= v.S || pr.reference < 0 || pr.reference >= v.S)
      return fail(COLATE_EINVAL, "pair %d: sample id out of range (target %d, reference %d, %d samples)", p, pr.target, pr.reference, v.S);
    if (pr.target_mask != -1 || pr.reference_mask != -1)
      return fail(COLATE_EINVAL, "pair %d: compare_tmp takes no masks (target mask %d, reference mask %d; both must be -1)", p,
                  pr.target_mask, pr.reference_mask);
  }
  long long total = 0;
  for (int c = 0; c < v.C; c++) {
    const long long nc = v.row_off[c + 1] - v.row_off[c];
    for (long long i = 0; i < nc; i++) {
      const int pos = v.rows[c][i].pos;
      if (pos < 0 || (i > 0 && pos < v.rows[c][i - 1].pos))
        return fail(COLATE_EINVAL, "chromosome %d, row %lld: position %d is negative or below the row in front (the walk index is one of ascending rows)", c, i, pos);
    }
    if (nc > 0 && v.first_pos[c] > v.rows[c][0].pos)
      return fail(COLATE_EINVAL, "chromosome %d: first_pos = %d above the first searched row's position %d", c, v.first_pos[c], v.rows[c][0].pos);
    if (nc > 0 && v.last_pos[c] < v.rows[c][nc - 1].pos)
      return fail(COLATE_EINVAL, "chromosome %d: last_pos = %d below the last searched row's position %d", c, v.last_pos[c], v.rows[c][nc - 1].pos);
    total += window_of(v.last_pos[c], v.first_pos[c], v.window) + 1;
    if (total > 0x7fffffffLL - v.C) return fail(COLATE_ELIMIT, "2^31 windows or more (window = %d)", v.window);
  }
  return COLATE_OK;
}

void window_rows(const View& v, std::vector<long long>& win_off, std::vector<int>& win_row) {
  win_off.assign((size_t)v.C + 1, 0);
  for (int c = 0; c < v.C; c++) win_off[(size_t)c + 1] = win_off[(size_t)c] + window_of(v.last_pos[c], v.first_pos[c], v.window) + 1;
  win_row.assign((size_t)(win_off[(size_t)v.C] + v.C), 0);
  for (int c = 0; c < v.C; c++) {
    const long long W = win_off[(size_t)c + 1] - win_off[(size_t)c], nc = v.row_off[c + 1] - v.row_off[c];
    int* const b = win_row.data() + win_off[(size_t)c] + c;
    long long i = 0;
    for (long long w = 0; w <= W; w++) {  // b[w]: the first row of window w or a later one
      while (w < W && i < nc && window_of(v.rows[c][i].pos, v.first_pos[c], v.window) < w) i++;
      b[w] = (int)(w < W ? i : nc);
    }
  }
}

void host_planes(const View& v, int s, const long long* word_off, long long words, unsigned long long* planes) {
  std::memset(planes, 0, sizeof(unsigned long long) * 2 * (size_t)words);
  for (int c = 0; c < v.C; c++) {
    const long long nc = v.row_off[c + 1] - v.row_off[c];
    const Idx* const X = v.idx[(size_t)s * v.C + c];
    for (long long i = 0; i < nc; i++) {
      const Idx x = X[i];
      if (!hits(x, i == 0 ? -1 : v.rows[c][i - 1].pos)) continue;
      const unsigned long long bit = 1ull << (i & 63);
      planes[word_off[c] + (i >> 6)] |= bit;
      if (fixed(x)) planes[words + word_off[c] + (i >> 6)] |= bit;
    }
  }
}

int check_outputs(long long cap, const long long* win_off, const int* mismatch, const int* snps) {
  if (!win_off) return fail(COLATE_EINVAL, "NULL pointer argument");
  if (cap < 0) return fail(COLATE_EINVAL, "cap = %lld is negative", cap);
  if (cap > 0 && (!mismatch || !snps)) return fail(COLATE_EINVAL, "NULL pointer argument");
  return COLATE_OK;
}

int check_capacity(long long P, long long windows, long long cap) {
  if (P * windows > cap)
    return fail(COLATE_ELIMIT, "%lld pairs of %lld windows, room for %lld counts (needed: %lld)", P, windows, cap, P * windows);
  return COLATE_OK;
}

int compare_view_host(const View& v, long long cap, long long* win_off, int* mismatch, int* snps) {
  if (int rc = check_outputs(cap, win_off, mismatch, snps)) return rc;
  if (int rc = check_view(v)) return rc;
  std::vector<long long> woff, word_off((size_t)v.C + 1);
  std::vector<int> win_row;
  window_rows(v, woff, win_row);
  const long long Wt = woff[(size_t)v.C];
  if (int rc = check_capacity(v.P, Wt, cap)) return rc;
  const long long words = colate_iw::mask_words(v.C, v.row_off, word_off.data());
  std::vector<unsigned long long> planes((size_t)v.S * 2 * (size_t)words);
  for (int s = 0; s < v.S; s++) host_planes(v, s, word_off.data(), words, planes.data() + (size_t)s * 2 * (size_t)words);
  for (int p = 0; p < v.P; p++) {
    const unsigned long long* const T = planes.data() + (size_t)v.pairs[p].target * 2 * (size_t)words;
    const unsigned long long* const R = planes.data() + (size_t)v.pairs[p].reference * 2 * (size_t)words;
    for (int c = 0; c < v.C; c++) {
      const int* const b = win_row.data() + woff[(size_t)c] + c;
      const long long W = woff[(size_t)c + 1] - woff[(size_t)c], w0 = word_off[(size_t)c];
      for (long long w = 0; w < W; w++) {
        int n = 0, mm = 0;
        const long long r0 = b[w], r1 = b[w + 1];
        for (long long k = r0 >> 6; r1 > r0 && k <= (r1 - 1) >> 6; k++) {
          const unsigned long long both = T[w0 + k] & R[w0 + k] & range_bits(k, r0, r1);
          n += __builtin_popcountll(both);
          mm += __builtin_popcountll(both & (T[words + w0 + k] ^ R[words + w0 + k]));
        }
        mismatch[(size_t)p * (size_t)Wt + (size_t)(woff[(size_t)c] + w)] = mm;
        snps[(size_t)p * (size_t)Wt + (size_t)(woff[(size_t)c] + w)] = n;
      }
    }
  }
  std::memcpy(win_off, woff.data(), sizeof(long long) * woff.size());
  return COLATE_OK;
}

namespace {

// the caller's back-to-back arrays, chromosome by chromosome
struct FlatView {
  View v;
  std::vector<const Row*> rows;
  std::vector<const Idx*> idx;
  FlatView(int C, const long long* row_off, const Row* r, int S, const Idx* x, int P, const Pair* pairs, const int* first_pos,
           const int* last_pos, int window) {
    v.C = C, v.row_off = row_off, v.S = S, v.P = P, v.pairs = pairs, v.first_pos = first_pos, v.last_pos = last_pos, v.window = window;
    bool ok = C >= 1 && S >= 1 && row_off && row_off[0] == 0;
    for (int c = 0; ok && c < C; c++) ok = row_off[c + 1] >= row_off[c];
    if (!ok) {  // (check_view names what is wrong with the sizes or offsets: nothing below is dereferenced before it)
      static const Row* const no_rows = nullptr;
      static const Idx* const no_idx = nullptr;
      v.rows = r ? &no_rows : nullptr, v.idx = x ? &no_idx : nullptr;
      return;
    }
    const long long n = row_off[C];
    rows.resize((size_t)C), idx.resize((size_t)S * C);
    for (int c = 0; c < C; c++) rows[(size_t)c] = r ? r + row_off[c] : nullptr;
    for (int s = 0; s < S; s++)
      for (int c = 0; c < C; c++) idx[(size_t)s * C + c] = x ? x + (size_t)s * n + row_off[c] : nullptr;
    v.rows = r ? rows.data() : nullptr, v.idx = x ? idx.data() : nullptr;
  }
};

}  // namespace

}  // namespace colate_cmp

using namespace colate_cmp;

extern "C" {

int colate_compare_samples_host(int C, const long long* row_off, const colate_walk_row* rows, int S, const colate_walk_idx* idx, int P,
                                const colate_walk_pair* pairs, const int* first_pos, const int* last_pos, int window, long long cap,
                                long long* win_off, int* mismatch, int* snps) {
  const FlatView f(C, row_off, rows, S, idx, P, pairs, first_pos, last_pos, window);
  return compare_view_host(f.v, cap, win_off, mismatch, snps);
}

int colate_compare_samples(int C, const long long* row_off, const colate_walk_row* rows, int S, const colate_walk_idx* idx, int P,
                           const colate_walk_pair* pairs, const int* first_pos, const int* last_pos, int window, long long cap,
                           long long* win_off, int* mismatch, int* snps) {
  const FlatView f(C, row_off, rows, S, idx, P, pairs, first_pos, last_pos, window);
  return compare_view_device(f.v, cap, win_off, mismatch, snps);
}

}  // extern "C"
