// colate_amd/csrc/count_topo.cpp -- the host side of colate_topo_samples (count_topo.h: the contract): the checks both forms run
// before anything is written; the host twins of the device calls -- HostPlanes builds every sample's bit planes once, and
// for_each_qualifying is the one walk over a triple's set bits of Q with the running rank; the ranked draws as planes
// (colate_topo_samples), binned by age (colate_topo_profile), by genome block and age (colate_topo_profile_blocks) and the expected
// counts in fixed point without a draw (colate_topo_expected_blocks) are a sink of that walk each --; the blocks themselves, the block
// jackknife on those counts (colate_topo_jackknife: host only), and the C entry points, which view the caller's back-to-back arrays
// chromosome by chromosome.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <vector>

#include "colate_amd.h"
#include "colate_internal.h"
#include "count_topo.h"

using colate::fail;

namespace colate_topo {

int check_view(const View& v) {
  if (v.C < 1 || v.S < 1 || v.P < 1)
    return fail(COLATE_EINVAL, "bad sizes C=%d S=%d P=%d (at least one chromosome, one sample and one triple)", v.C, v.S, v.P);
  if (!v.row_off) return fail(COLATE_EINVAL, "NULL pointer argument");
  if (v.n_uniforms < 0) return fail(COLATE_EINVAL, "n_uniforms = %lld is negative", v.n_uniforms);
  if (v.n_uniforms > 0 && !v.uniforms) return fail(COLATE_EINVAL, "NULL pointer argument");
  if (v.row_off[0] != 0) return fail(COLATE_EINVAL, "row_off[0] = %lld must be 0", v.row_off[0]);
  for (int c = 0; c < v.C; c++) {
    if (v.row_off[c + 1] < v.row_off[c])
      return fail(COLATE_EINVAL, "row_off decreases at chromosome %d (%lld after %lld)", c, v.row_off[c + 1], v.row_off[c]);
    if (v.row_off[c + 1] - v.row_off[c] > 0x7fffffffLL) return fail(COLATE_ELIMIT, "chromosome %d has 2^31 rows or more", c);
  }
  if (!v.rows || !v.idx || !v.cidx || !v.triples) return fail(COLATE_EINVAL, "NULL pointer argument");
  for (int c = 0; c < v.C; c++)
    if (v.row_off[c + 1] > v.row_off[c] && !v.rows[c]) return fail(COLATE_EINVAL, "NULL pointer argument");
  for (size_t k = 0; k < (size_t)v.S * v.C; k++)
    if (v.row_off[k % v.C + 1] > v.row_off[k % v.C] && (!v.idx[k] || !v.cidx[k])) return fail(COLATE_EINVAL, "NULL pointer argument");
  for (int p = 0; p < v.P; p++) {
    const Triple& t = v.triples[p];
    if (t.cond < 0 || t.cond >= v.S || t.target < 0 || t.target >= v.S || t.reference < 0 || t.reference >= v.S)
      return fail(COLATE_EINVAL, "triple %d: sample id out of range (cond %d, target %d, reference %d, %d samples)", p, t.cond, t.target,
                  t.reference, v.S);
  }
  for (int c = 0; c < v.C; c++) {
    const long long nc = v.row_off[c + 1] - v.row_off[c];
    for (long long i = 0; i < nc; i++) {
      const int pos = v.rows[c][i].pos;
      if (pos < 0 || (i > 0 && pos < v.rows[c][i - 1].pos))
        return fail(COLATE_EINVAL, "chromosome %d, row %lld: position %d is negative or below the row in front (the walk index is one of ascending rows)", c, i, pos);
    }
  }
  return COLATE_OK;
}

int check_outputs(long long cap, const long long* word_off, const unsigned long long* plus, const unsigned long long* minus, const long long* draws) {
  if (!word_off || !draws) return fail(COLATE_EINVAL, "NULL pointer argument");
  if (cap < 0) return fail(COLATE_EINVAL, "cap = %lld is negative", cap);
  if (cap > 0 && (!plus || !minus)) return fail(COLATE_EINVAL, "NULL pointer argument");
  return COLATE_OK;
}

int check_capacity(long long P, long long words, long long cap) {
  if (P * words > cap)
    return fail(COLATE_ELIMIT, "%lld triples of %lld words, room for %lld words per plane (needed: %lld)", P, words, cap, P * words);
  return COLATE_OK;
}

int check_stream(const View& v, const long long* draws) {
  long long most = 0;
  int at = 0;
  for (int p = 0; p < v.P; p++)
    if (draws[p] > most) most = draws[p], at = p;
  if (2 * most > v.n_uniforms)
    return fail(COLATE_ELIMIT, "triple %d has %lld qualifying rows, the stream holds %lld uniforms (needed: %lld)", at, most, v.n_uniforms, 2 * most);
  return COLATE_OK;
}

namespace {

// Every sample's two bit planes over the searched rows -- `hit` from its walk index, `qualifies` from its cond index, every
// chromosome starting on a word -- and from them a triple's Q: the host's form of what the planes kernel writes.
struct HostPlanes {
  const View& v;
  std::vector<long long> woff;
  long long words;
  std::vector<unsigned long long> bits;  // [S][2][words]
  explicit HostPlanes(const View& view) : v(view), woff((size_t)view.C + 1) {
    words = colate_iw::mask_words(v.C, v.row_off, woff.data());
    bits.assign((size_t)v.S * 2 * (size_t)words, 0);
    for (int s = 0; s < v.S; s++)
      for (int c = 0; c < v.C; c++) {
        const long long nc = v.row_off[c + 1] - v.row_off[c];
        const Idx* const X = v.idx[(size_t)s * v.C + c];
        const Idx* const Y = v.cidx[(size_t)s * v.C + c];
        unsigned long long* const hit = bits.data() + (size_t)s * 2 * (size_t)words + woff[(size_t)c];
        unsigned long long* const qual = hit + words;
        for (long long i = 0; i < nc; i++) {
          const unsigned long long bit = 1ull << (i & 63);
          if (hits(X[i])) hit[i >> 6] |= bit;
          if (qualifies(Y[i])) qual[i >> 6] |= bit;
        }
      }
  }
  const unsigned long long* plane(int s, int which) const { return bits.data() + ((size_t)s * 2 + (size_t)which) * (size_t)words; }
  // the three planes of triple p; Q at word k is their conjunction
  struct OfTriple {
    const unsigned long long *T, *R, *Cq;
    unsigned long long operator()(long long k) const { return T[k] & R[k] & Cq[k]; }
  };
  OfTriple of(int p) const { return OfTriple{plane(v.triples[p].target, 0), plane(v.triples[p].reference, 0), plane(v.triples[p].cond, 1)}; }
  long long qualifying(int p) const {
    const OfTriple q = of(p);
    long long n = 0;
    for (long long k = 0; k < words; k++) n += __builtin_popcountll(q(k));
    return n;
  }
  // the count pass of the forms that draw: the stream is checked before anything is written
  int check_stream() const {
    std::vector<long long> n((size_t)v.P);
    for (int p = 0; p < v.P; p++) n[(size_t)p] = qualifying(p);
    return colate_topo::check_stream(v, n.data());
  }
};

// The one walk over the qualifying rows of triple p, in the genome's order: sink(c, i, rank, T, R) at row i of chromosome c, the
// triple's qualifying row number `rank` -- a running popcount -- with the index entries of its target and its reference there.
// Returns the number of those rows.
template <class Sink>
long long for_each_qualifying(const View& v, const HostPlanes& planes, int p, Sink&& sink) {
  const Triple& t = v.triples[p];
  const HostPlanes::OfTriple q = planes.of(p);
  long long rank = 0;
  for (int c = 0; c < v.C; c++) {
    const Idx* const TI = v.idx[(size_t)t.target * v.C + c];
    const Idx* const RI = v.idx[(size_t)t.reference * v.C + c];
    const long long w0 = planes.woff[(size_t)c];
    for (long long k = w0; k < planes.woff[(size_t)c + 1]; k++)
      for (unsigned long long w = q(k); w; w &= w - 1, rank++) {
        const long long i = (k - w0) * 64 + __builtin_ctzll(w);
        sink(c, i, rank, TI[i], RI[i]);
      }
  }
  return rank;
}

// The profile twins' sink: the draw of every qualifying row counted in counts[P][nb][E][3] at the row's block -- block_of(c, row) --
// and epoch: qualifying, and plus or minus by its sign.  The rank runs on across blocks and chromosomes.
template <class BlockOf>
void draw_profile(const View& v, const HostPlanes& planes, int E, const double* epochs, size_t nb, BlockOf&& block_of, long long* counts,
                  long long* draws) {
  const size_t per_block = (size_t)E * 3;
  std::memset(counts, 0, sizeof(long long) * (size_t)v.P * nb * per_block);
  for (int p = 0; p < v.P; p++) {
    long long* const mine = counts + (size_t)p * nb * per_block;
    draws[p] = for_each_qualifying(v, planes, p, [&](int c, long long i, long long rank, const Idx& T, const Idx& R) {
      const Row& m = v.rows[c][i];
      const int sign = draw_sign(T, R, v.uniforms[2 * rank], v.uniforms[2 * rank + 1]);
      long long* const at = mine + block_of(c, m) * per_block + (size_t)age_epoch(m.age_begin, m.age_end, epochs, E) * 3;
      at[2]++;
      if (sign > 0) at[0]++;
      if (sign < 0) at[1]++;
    });
  }
}

}  // namespace

int topo_view_host(const View& v, long long cap, long long* word_off, unsigned long long* plus, unsigned long long* minus, long long* draws) {
  if (int rc = check_outputs(cap, word_off, plus, minus, draws)) return rc;
  if (int rc = check_view(v)) return rc;
  if (int rc = check_capacity(v.P, colate_iw::mask_words(v.C, v.row_off, nullptr), cap)) return rc;
  const HostPlanes planes(v);
  if (int rc = planes.check_stream()) return rc;
  const size_t words = (size_t)planes.words;
  std::fill_n(plus, (size_t)v.P * words, 0ull), std::fill_n(minus, (size_t)v.P * words, 0ull);
  for (int p = 0; p < v.P; p++) {
    unsigned long long* const pl = plus + (size_t)p * words;
    unsigned long long* const mi = minus + (size_t)p * words;
    draws[p] = for_each_qualifying(v, planes, p, [&](int c, long long i, long long rank, const Idx& T, const Idx& R) {
      const int sign = draw_sign(T, R, v.uniforms[2 * rank], v.uniforms[2 * rank + 1]);
      const long long k = planes.woff[(size_t)c] + (i >> 6);
      if (sign > 0) pl[k] |= 1ull << (i & 63);
      if (sign < 0) mi[k] |= 1ull << (i & 63);
    });
  }
  std::memcpy(word_off, planes.woff.data(), sizeof(long long) * planes.woff.size());
  return COLATE_OK;
}

int check_epochs(int E, const double* epochs) {
  if (E < 1 || E > kMaxProfileEpochs) return fail(COLATE_EINVAL, "E = %d epochs: 1 to %d are possible", E, kMaxProfileEpochs);
  if (!epochs) return fail(COLATE_EINVAL, "NULL pointer argument");
  for (int e = 0; e < E; e++) {
    if (!std::isfinite(epochs[e])) return fail(COLATE_EINVAL, "epochs[%d] is not finite", e);
    if (e > 0 && !(epochs[e] > epochs[e - 1]))
      return fail(COLATE_EINVAL, "epochs[%d] = %g does not lie above epochs[%d] = %g (the epochs ascend strictly)", e, epochs[e], e - 1, epochs[e - 1]);
  }
  return COLATE_OK;
}

int topo_profile_host(const View& v, int E, const double* epochs, long long* counts, long long* draws) {
  if (!counts || !draws) return fail(COLATE_EINVAL, "NULL pointer argument");
  if (int rc = check_epochs(E, epochs)) return rc;
  if (int rc = check_view(v)) return rc;
  const HostPlanes planes(v);
  if (int rc = planes.check_stream()) return rc;
  draw_profile(v, planes, E, epochs, 1, [](int, const Row&) { return (size_t)0; }, counts, draws);
  return COLATE_OK;
}

int block_offsets(int C, const int* max_pos, int nbpb, int* blk_off) {
  if (C < 1) return fail(COLATE_EINVAL, "bad sizes C=%d (at least one chromosome)", C);
  if (!max_pos || !blk_off) return fail(COLATE_EINVAL, "NULL pointer argument");
  if (nbpb < 1) return fail(COLATE_EINVAL, "num_bases_per_block = %d: at least 1", nbpb);
  long long nb = 0;
  for (int c = 0; c < C; c++) {
    if ((long long)max_pos[c] >= (1LL << 31) - nbpb)
      return fail(COLATE_EINVAL, "chromosome %d: position %d at or above 2^31 - num_bases_per_block (%d)", c, max_pos[c], nbpb);
    nb += block_of_pos(max_pos[c], nbpb) + 1;
  }
  if (nb > kMaxTopoBlocks)
    return fail(COLATE_ELIMIT, "%lld blocks of %d bases, %d are possible (needed: %lld)", nb, nbpb, kMaxTopoBlocks, nb);
  blk_off[0] = 0;
  for (int c = 0; c < C; c++) blk_off[c + 1] = blk_off[c] + block_of_pos(max_pos[c], nbpb) + 1;
  return COLATE_OK;
}

int topo_blocks(int C, const long long* row_off, const Row* const* rows, int nbpb, int* blk_off) {
  if (C < 1) return fail(COLATE_EINVAL, "bad sizes C=%d (at least one chromosome)", C);
  if (!row_off || !blk_off) return fail(COLATE_EINVAL, "NULL pointer argument");
  if (row_off[0] != 0) return fail(COLATE_EINVAL, "row_off[0] = %lld must be 0", row_off[0]);
  for (int c = 0; c < C; c++)
    if (row_off[c + 1] < row_off[c])
      return fail(COLATE_EINVAL, "row_off decreases at chromosome %d (%lld after %lld)", c, row_off[c + 1], row_off[c]);
  if (row_off[C] > 0 && !rows) return fail(COLATE_EINVAL, "NULL pointer argument");
  std::vector<int> max_pos((size_t)C, 0);
  for (int c = 0; c < C; c++) {
    const long long nc = row_off[c + 1] - row_off[c];
    if (nc > 0 && !rows[c]) return fail(COLATE_EINVAL, "NULL pointer argument");
    for (long long i = 0; i < nc; i++) max_pos[(size_t)c] = std::max(max_pos[(size_t)c], rows[c][i].pos);
  }
  return block_offsets(C, max_pos.data(), nbpb, blk_off);
}

int check_blocks(const View& v, int E, int nbpb, int nb, std::vector<int>& blk_off) {
  blk_off.assign((size_t)v.C + 1, 0);
  if (int rc = topo_blocks(v.C, v.row_off, v.rows, nbpb, blk_off.data())) return rc;
  if (nb != blk_off[(size_t)v.C])
    return fail(COLATE_EINVAL, "nb = %d is not the %d blocks of these rows at %d bases per block (colate_topo_blocks)", nb, blk_off[(size_t)v.C], nbpb);
  const long long bytes = 12LL * E * nb;
  if (bytes > kMaxBlockPartialBytes)
    return fail(COLATE_ELIMIT, "%d epochs x %d blocks: %lld bytes of partials per triple, %lld are possible", E, nb, bytes, kMaxBlockPartialBytes);
  return COLATE_OK;
}

void block_segments(const View& v, int nbpb, const int* blk_off, Segment* seg) {
  for (int c = 0; c < v.C; c++) {
    const Row* const r = v.rows[c];
    const long long nc = v.row_off[c + 1] - v.row_off[c];
    const int nbc = blk_off[c + 1] - blk_off[c];
    long long first = 0;  // (positions ascend: the rows of block k are those between two partition points)
    for (int k = 0; k < nbc; k++) {
      const long long end =
          k + 1 == nbc ? nc : std::partition_point(r + first, r + nc, [&](const Row& m) { return block_of_pos(m.pos, nbpb) <= k; }) - r;
      seg[blk_off[c] + k] = Segment{c, (int)first, (int)end};
      first = end;
    }
  }
}

int topo_profile_blocks_host(const View& v, int E, const double* epochs, int nbpb, int nb, long long* counts, long long* draws) {
  if (!counts || !draws) return fail(COLATE_EINVAL, "NULL pointer argument");
  if (int rc = check_epochs(E, epochs)) return rc;
  if (int rc = check_view(v)) return rc;
  std::vector<int> blk_off;
  if (int rc = check_blocks(v, E, nbpb, nb, blk_off)) return rc;
  const HostPlanes planes(v);
  if (int rc = planes.check_stream()) return rc;
  // the row's position names the block
  draw_profile(v, planes, E, epochs, (size_t)nb, [&](int c, const Row& m) { return (size_t)(blk_off[(size_t)c] + block_of_pos(m.pos, nbpb)); },
               counts, draws);
  return COLATE_OK;
}

int check_expected(const View& v, int E, const double* epochs, int nbpb, int nb, const long long* counts, std::vector<int>& blk_off) {
  if (!counts) return fail(COLATE_EINVAL, "NULL pointer argument");
  if (int rc = check_epochs(E, epochs)) return rc;
  View w = v;
  w.n_uniforms = 0, w.uniforms = nullptr;  // (no stream goes in)
  if (int rc = check_view(w)) return rc;
  if (int rc = check_blocks(v, E, nbpb, nb, blk_off)) return rc;
  if (v.row_off[v.C] > kMaxExpectedRows)
    return fail(COLATE_ELIMIT, "%lld searched rows, %lld are possible (the sums of the expected counts stay below 2^62)", v.row_off[v.C], kMaxExpectedRows);
  return COLATE_OK;
}

int topo_expected_blocks_host(const View& v, int E, const double* epochs, int nbpb, int nb, long long* counts) {
  std::vector<int> blk_off;
  if (int rc = check_expected(v, E, epochs, nbpb, nb, counts, blk_off)) return rc;
  const HostPlanes planes(v);
  // a row's addends depend on that row alone: no stream, no rank
  const size_t per_block = (size_t)E * 3;
  std::memset(counts, 0, sizeof(long long) * (size_t)v.P * (size_t)nb * per_block);
  for (int p = 0; p < v.P; p++) {
    long long* const mine = counts + (size_t)p * (size_t)nb * per_block;
    for_each_qualifying(v, planes, p, [&](int c, long long i, long long, const Idx& T, const Idx& R) {
      const Row& m = v.rows[c][i];
      const Addends x = expected_addends(T, R);
      const size_t b = (size_t)(blk_off[(size_t)c] + block_of_pos(m.pos, nbpb));
      long long* const at = mine + b * per_block + (size_t)age_epoch(m.age_begin, m.age_end, epochs, E) * 3;
      at[0] += (long long)x.plus, at[1] += (long long)x.minus, at[2]++;
    });
  }
  return COLATE_OK;
}

void jackknife(int nb, int E, const long long* counts, double* out, int* used) {
  const double na = std::numeric_limits<double>::quiet_NaN();
  std::vector<long long> a((size_t)nb), b((size_t)nb);
  for (int cell = 0; cell <= E; cell++) {
    long long A = 0, M = 0;
    int g = 0;
    for (int j = 0; j < nb; j++) {
      long long aj = 0, bj = 0;
      for (int e = cell < E ? cell : 0; e < (cell < E ? cell + 1 : E); e++)
        aj += counts[((size_t)j * E + e) * 3], bj += counts[((size_t)j * E + e) * 3 + 1];
      a[(size_t)j] = aj, b[(size_t)j] = bj, A += aj, M += bj, g += aj + bj > 0;
    }
    double* const o = out + (size_t)cell * 4;
    o[0] = o[1] = o[2] = o[3] = na, used[cell] = g;
    const long long n = A + M;
    if (n == 0) continue;
    const double D = (double)(A - M) / (double)n;
    o[0] = D;
    if (g < 2) continue;
    auto theta = [&](size_t j) { return (double)((A - a[j]) - (M - b[j])) / (double)(n - (a[j] + b[j])); };
    double s = 0.0;
    for (size_t j = 0; j < (size_t)nb; j++) {
      const long long nj = a[j] + b[j];
      if (nj > 0) s += ((double)(n - nj) / (double)n) * theta(j);
    }
    const double D_jack = (double)g * D - s;
    double var = 0.0;
    for (size_t j = 0; j < (size_t)nb; j++) {
      const long long nj = a[j] + b[j];
      if (nj == 0) continue;
      const double h = (double)n / (double)nj;
      const double tau = h * D - (h - 1.0) * theta(j);
      const double d = tau - D_jack;
      var += (d * d) / (h - 1.0);
    }
    const double se = std::sqrt(var / (double)g);
    o[1] = D_jack, o[2] = se, o[3] = se > 0 ? D_jack / se : na;
  }
}

namespace {

// Whether the caller's offsets can be followed at all: where not, the checks name what is wrong with the sizes or offsets, and
// nothing is dereferenced before them.
bool offsets_usable(int C, const long long* row_off) {
  bool ok = C >= 1 && row_off && row_off[0] == 0;
  for (int c = 0; ok && c < C; c++) ok = row_off[c + 1] >= row_off[c];
  return ok;
}

// the caller's back-to-back arrays, chromosome by chromosome
struct FlatView {
  View v;
  std::vector<const Row*> rows;
  std::vector<const Idx*> idx, cidx;
  FlatView(int C, const long long* row_off, const Row* r, int S, const Idx* x, const Idx* y, int P, const Triple* triples, long long n_uniforms,
           const double* uniforms) {
    v.C = C, v.row_off = row_off, v.S = S, v.P = P, v.triples = triples, v.n_uniforms = n_uniforms, v.uniforms = uniforms;
    if (S < 1 || !offsets_usable(C, row_off)) {  // (check_view names what is wrong)
      static const Row* const no_rows = nullptr;
      static const Idx* const no_idx = nullptr;
      v.rows = r ? &no_rows : nullptr, v.idx = x ? &no_idx : nullptr, v.cidx = y ? &no_idx : nullptr;
      return;
    }
    const long long n = row_off[C];
    rows.resize((size_t)C), idx.resize((size_t)S * C), cidx.resize((size_t)S * C);
    for (int c = 0; c < C; c++) rows[(size_t)c] = r ? r + row_off[c] : nullptr;
    for (int s = 0; s < S; s++)
      for (int c = 0; c < C; c++) {
        idx[(size_t)s * C + c] = x ? x + (size_t)s * n + row_off[c] : nullptr;
        cidx[(size_t)s * C + c] = y ? y + (size_t)s * n + row_off[c] : nullptr;
      }
    v.rows = r ? rows.data() : nullptr, v.idx = x ? idx.data() : nullptr, v.cidx = y ? cidx.data() : nullptr;
  }
};

}  // namespace

}  // namespace colate_topo

using namespace colate_topo;

extern "C" {

int colate_topo_samples_host(int C, const long long* row_off, const colate_walk_row* rows, int S, const colate_walk_idx* idx,
                             const colate_walk_idx* cond_idx, int P, const colate_topo_triple* triples, long long n_uniforms,
                             const double* uniforms, long long cap, long long* word_off, unsigned long long* plus, unsigned long long* minus,
                             long long* draws) {
  const FlatView f(C, row_off, rows, S, idx, cond_idx, P, triples, n_uniforms, uniforms);
  return topo_view_host(f.v, cap, word_off, plus, minus, draws);
}

int colate_topo_samples(int C, const long long* row_off, const colate_walk_row* rows, int S, const colate_walk_idx* idx,
                        const colate_walk_idx* cond_idx, int P, const colate_topo_triple* triples, long long n_uniforms, const double* uniforms,
                        long long cap, long long* word_off, unsigned long long* plus, unsigned long long* minus, long long* draws) {
  const FlatView f(C, row_off, rows, S, idx, cond_idx, P, triples, n_uniforms, uniforms);
  return topo_view_device(f.v, cap, word_off, plus, minus, draws);
}

int colate_topo_profile_host(int C, const long long* row_off, const colate_walk_row* rows, int S, const colate_walk_idx* idx,
                             const colate_walk_idx* cond_idx, int P, const colate_topo_triple* triples, long long n_uniforms,
                             const double* uniforms, int E, const double* epochs, long long* counts, long long* draws) {
  const FlatView f(C, row_off, rows, S, idx, cond_idx, P, triples, n_uniforms, uniforms);
  return topo_profile_host(f.v, E, epochs, counts, draws);
}

int colate_topo_profile(int C, const long long* row_off, const colate_walk_row* rows, int S, const colate_walk_idx* idx,
                        const colate_walk_idx* cond_idx, int P, const colate_topo_triple* triples, long long n_uniforms, const double* uniforms,
                        int E, const double* epochs, long long* counts, long long* draws) {
  const FlatView f(C, row_off, rows, S, idx, cond_idx, P, triples, n_uniforms, uniforms);
  return topo_profile_device(f.v, E, epochs, counts, draws);
}

int colate_topo_blocks(int C, const long long* row_off, const colate_walk_row* rows, int num_bases_per_block, int* blk_off) {
  std::vector<const Row*> ptrs;
  if (offsets_usable(C, row_off) && rows)  // (topo_blocks names what is wrong)
    for (int c = 0; c < C; c++) ptrs.push_back(rows + row_off[c]);
  return topo_blocks(C, row_off, ptrs.empty() ? nullptr : ptrs.data(), num_bases_per_block, blk_off);
}

int colate_topo_profile_blocks_host(int C, const long long* row_off, const colate_walk_row* rows, int S, const colate_walk_idx* idx,
                                    const colate_walk_idx* cond_idx, int P, const colate_topo_triple* triples, long long n_uniforms,
                                    const double* uniforms, int E, const double* epochs, int num_bases_per_block, int nb, long long* counts,
                                    long long* draws) {
  const FlatView f(C, row_off, rows, S, idx, cond_idx, P, triples, n_uniforms, uniforms);
  return topo_profile_blocks_host(f.v, E, epochs, num_bases_per_block, nb, counts, draws);
}

int colate_topo_profile_blocks(int C, const long long* row_off, const colate_walk_row* rows, int S, const colate_walk_idx* idx,
                               const colate_walk_idx* cond_idx, int P, const colate_topo_triple* triples, long long n_uniforms,
                               const double* uniforms, int E, const double* epochs, int num_bases_per_block, int nb, long long* counts,
                               long long* draws) {
  const FlatView f(C, row_off, rows, S, idx, cond_idx, P, triples, n_uniforms, uniforms);
  return topo_profile_blocks_device(f.v, E, epochs, num_bases_per_block, nb, counts, draws);
}

int colate_topo_expected_blocks_host(int C, const long long* row_off, const colate_walk_row* rows, int S, const colate_walk_idx* idx,
                                     const colate_walk_idx* cond_idx, int P, const colate_topo_triple* triples, int E, const double* epochs,
                                     int num_bases_per_block, int nb, long long* counts) {
  const FlatView f(C, row_off, rows, S, idx, cond_idx, P, triples, 0, nullptr);
  return topo_expected_blocks_host(f.v, E, epochs, num_bases_per_block, nb, counts);
}

int colate_topo_expected_blocks(int C, const long long* row_off, const colate_walk_row* rows, int S, const colate_walk_idx* idx,
                                const colate_walk_idx* cond_idx, int P, const colate_topo_triple* triples, int E, const double* epochs,
                                int num_bases_per_block, int nb, long long* counts) {
  const FlatView f(C, row_off, rows, S, idx, cond_idx, P, triples, 0, nullptr);
  return topo_expected_blocks_device(f.v, E, epochs, num_bases_per_block, nb, counts);
}

int colate_topo_jackknife(int nb, int E, const long long* counts, double* out, int* used) {
  if (nb < 1 || E < 1) return fail(COLATE_EINVAL, "bad sizes nb=%d E=%d (at least one block and one epoch)", nb, E);
  if (!counts || !out || !used) return fail(COLATE_EINVAL, "NULL pointer argument");
  for (size_t k = 0; k < (size_t)nb * (size_t)E * 3; k++)
    if (counts[k] < 0) return fail(COLATE_EINVAL, "counts[%zu] = %lld is negative", k, counts[k]);
  jackknife(nb, E, counts, out, used);
  return COLATE_OK;
}

int colate_topo_samples_tile(void) { return kTileRows; }

}  // extern "C"
