// colate_amd/csrc/fill_samples.cpp -- the host side of colate_fill_samples (fill_samples.h: the contract): the checks of both
// forms, the host twin -- a plain loop per pair with a std::mt19937 of its own, the logarithm of age_bin_index and the redraw
// loop of coal.cpp:2279-2295, so it is right for every input --, the chunk plan of the device form, the C entry points, and
// fill_sample_pairs, the fill of `Colate --mode mut --samples` around the device form (mut_inputs.h).
#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <random>
#include <string>
#include <vector>

#include "age_bins.hpp"
#include "cli_lists.h"
#include "colate_amd.h"
#include "colate_internal.h"
#include "fill_samples.h"
#include "interval_walk.h"
#include "uniform_stream.hpp"
#include "walk_inputs.h"

using colate::fail;
using colate_drv::FillRec;
using namespace colate_iw;

namespace colate_fs {

int check_fill(const View& v, int A) {
  if (A != colate_ic::kBins) return fail(COLATE_EINVAL, "A = %d: the fill takes the %d bins of colate_age_grid", A, colate_ic::kBins);
  return check_view(v);
}

int size_result(const View& v, int A, const int* cnt, const int* last, std::vector<int>& blk0, Result& out) {
  const size_t P = (size_t)v.P;
  std::vector<long long> rec_off(P + 1);
  blk0.resize(P * v.C), out.nb.resize(P);
  if (int rc = finish_counts(v.P, v.C, cnt, last, blk0.data(), out.nb.data(), rec_off.data())) return rc;
  out.used.resize(P), out.table_off.assign(P + 1, 0), out.words.assign(P, 0), out.handed_back.assign(P, 0), out.near_band.assign(P, 0);
  for (size_t p = 0; p < P; p++) {
    out.used[p] = rec_off[p + 1] - rec_off[p];
    out.table_off[p + 1] = out.table_off[p] + (size_t)out.nb[p] * 4 * (size_t)A;
  }
  out.tables.assign(out.table_off[P], 0.0);
  return COLATE_OK;
}

namespace {
// inside the guard band of a located step: lo[k] <= x < hi[k] for some k in 1 .. A (the bands do not overlap and ascend)
bool in_band(const colate_drv::FastBin* bands, int A, double x) {
  if (!bands) return false;
  const double* lo = bands->guard_lo();
  const double* hi = bands->guard_hi();
  const int k = (int)(std::upper_bound(lo + 1, lo + A + 1, x) - lo) - 1;  // the last k with lo[k] <= x (0: none)
  return k >= 1 && x < hi[k];
}
}  // namespace

void twin_pair(const View& v, int p, int A, unsigned seed, const int* blk0, const colate_drv::FastBin* bands, Result& out) {
  const double C = 10.0, age = 0.0;
  const size_t n = (size_t)out.used[(size_t)p];
  std::vector<FillRec> recs(n);
  std::vector<FillSide> side(n);
  std::vector<int> block(n);
  host_write_fill(v, p, blk0, recs.data(), side.data(), block.data());
  double* const tab = out.tables.data() + out.table_off[(size_t)p];
  std::fill(tab, tab + (size_t)out.nb[(size_t)p] * 4 * (size_t)A, 0.0);
  std::mt19937 rng(seed);
  std::uniform_real_distribution<double> dist_unif(0, 1);
  unsigned long long draws = 0;
  bool near = false;
  for (size_t i = 0; i < n; i++) {
    const FillRec& s = recs[i];
    double* const t = tab + (size_t)block[i] * 4 * (size_t)A;
    const double begin = s.begin, span = (double)s.end - begin;
    if (begin <= age) {  // coal.cpp:2247-2275
      const int bin2 = colate_drv::age_bin_index(s.end, C);
      if (bin2 < A) t[2 * A + bin2] += side[i].e_sh, t[3 * A + bin2] += side[i].e_ns;
      for (int j = 0; j < kDraws; j++, draws++) {
        double sampled_age = dist_unif(rng) * span + begin;
        near = near || in_band(bands, A, sampled_age);
        if (sampled_age < age) sampled_age = age;
        const int bin = colate_drv::age_bin_index(sampled_age, C);
        if (bin < A) t[A + bin] += s.w_ns;
      }
    } else {  // coal.cpp:2279-2295
      int j = 0;
      while (j < kDraws) {
        const double sampled_age = dist_unif(rng) * span + begin;
        draws++;
        near = near || in_band(bands, A, sampled_age);
        const int bin = colate_drv::age_bin_index(sampled_age, C);
        if (sampled_age < age || bin >= A) {  // drawn again
          near = true;
          if (!(span == span) || !(begin == begin) || draws > 100ull * kDraws * (n + 1)) break;  // (no age in range can come: the reference never ends)
          continue;
        }
        t[bin] += s.w_sh, t[A + bin] += s.w_ns;
        j++;
      }
    }
  }
  out.words[(size_t)p] = 2 * draws;
  out.near_band[(size_t)p] = near ? 1 : 0;
}

std::vector<std::pair<int, int>> plan_chunks(int P, const long long* rec_off, long long budget_recs) {
  std::vector<std::pair<int, int>> chunks;
  for (int p0 = 0; p0 < P;) {
    int p1 = p0 + 1;
    while (p1 < P && rec_off[p1 + 1] - rec_off[p0] <= budget_recs) p1++;
    chunks.emplace_back(p0, p1);
    p0 = p1;
  }
  return chunks;
}

int fill_view_host(const View& v, int A, unsigned seed, Result& out) {
  if (int rc = check_fill(v, A)) return rc;
  const size_t PC = (size_t)v.P * v.C;
  std::vector<int> cnt(PC), last(PC), blk0;
  for (int p = 0; p < v.P; p++) host_count(v, p, cnt.data() + (size_t)p * v.C, last.data() + (size_t)p * v.C);
  if (int rc = size_result(v, A, cnt.data(), last.data(), blk0, out)) return rc;
  const colate_drv::FastBin bands(A, 10.0);
  for (int p = 0; p < v.P; p++) twin_pair(v, p, A, seed, blk0.data() + (size_t)p * v.C, bands.ok() ? &bands : nullptr, out);
  out.chunks = 0, out.kernel_s = 0.0;
  return COLATE_OK;
}

namespace {

// the caller's back-to-back arrays, chromosome by chromosome (the pointers live in the object; what is wrong with the sizes or
// offsets is left for check_view to name: nothing is dereferenced before it)
struct FlatView {
  View v;
  std::vector<const Row*> rows;
  std::vector<const Idx*> idx;
  std::vector<const unsigned long long*> masks;
  FlatView(int C, const long long* row_off, const Row* r, int S, const Idx* x, int M, const unsigned long long* m, int P, const Pair* pairs,
           int nbpb) {
    v.C = C, v.row_off = row_off, v.S = S, v.M = M, v.P = P, v.pairs = pairs, v.nbpb = nbpb;
    bool ok = C >= 1 && S >= 1 && M >= 0 && row_off && row_off[0] == 0;
    for (int c = 0; ok && c < C; c++) ok = row_off[c + 1] >= row_off[c];
    if (!ok) {
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

thread_local int g_chunks = 0;
thread_local double g_kernel_s = 0.0;

int fill_call(bool device, const FlatView& f, int A, unsigned seed, long long cap_blocks, int* out_nb, long long* out_used, double* out_tables,
              unsigned long long* out_words, int* out_handed_back, int* out_near_band) {
  if (!out_nb || !out_used || !out_words || !out_handed_back || (!device && !out_near_band)) return fail(COLATE_EINVAL, "NULL pointer argument");
  if (cap_blocks < 0) return fail(COLATE_EINVAL, "cap_blocks = %lld is negative", cap_blocks);
  if (cap_blocks > 0 && !out_tables) return fail(COLATE_EINVAL, "NULL pointer argument");
  Result res;
  if (int rc = device ? fill_view_device(f.v, A, seed, res) : fill_view_host(f.v, A, seed, res)) return rc;
  const size_t P = (size_t)f.v.P;
  const long long blocks = (long long)(res.table_off[P] / (4 * (size_t)A));
  if (blocks > cap_blocks)
    return fail(COLATE_ELIMIT, "the pairs have %lld genome blocks, room for %lld (needed: %lld)", blocks, cap_blocks, blocks);
  std::memcpy(out_nb, res.nb.data(), sizeof(int) * P), std::memcpy(out_used, res.used.data(), sizeof(long long) * P);
  if (!res.tables.empty()) std::memcpy(out_tables, res.tables.data(), sizeof(double) * res.tables.size());
  std::memcpy(out_words, res.words.data(), sizeof(unsigned long long) * P);
  std::memcpy(out_handed_back, res.handed_back.data(), sizeof(int) * P);
  if (out_near_band) std::memcpy(out_near_band, res.near_band.data(), sizeof(int) * P);
  g_chunks = res.chunks, g_kernel_s = res.kernel_s;
  return COLATE_OK;
}

}  // namespace

}  // namespace colate_fs

namespace colate_drv {

// (mut_inputs.h)
bool fill_sample_pairs(const Options& opt, const std::vector<std::string>& names, const std::vector<std::string>& mut_files,
                       const std::vector<PairSpec>& pairs, const std::vector<size_t>& todo, int seed, int A, std::vector<PairTables>& out) {
  const auto through_engine = [&](const char* why) {
    std::cerr << "pairs walked and filled through the engine of --pairs (" << why << ")" << std::endl;
    return fill_pairs(opt, names, mut_files, pairs, todo, seed, A, out);
  };
  for (const char* name : {"COLATE_DEVICE_FILL", "COLATE_DEVICE_FILL_WALK"})
    if (const char* e = std::getenv(name))
      if (std::atoi(e) == 0) return through_engine((std::string(name) + "=0").c_str());
  std::string why;
  if (choose_path(nullptr, true, why) != Path::device) return through_engine(why.c_str());
  if (!bind_device(opt)) return false;
  const double t0 = StageTimes::now();
  std::vector<PairSpec> mine;
  for (size_t p : todo) mine.push_back(pairs[p]);
  WalkInputs in;
  if (!load_walk_inputs(names, mut_files, mine, in)) return false;
  if (!in.indexed) return through_engine("a sample has no walk index");
  const View v = in.walk_view(kIntervalBasesPerBlock);
  const double t1 = StageTimes::now();
  colate_fs::Result res;
  if (int rc = colate_fs::fill_view_device(v, A, (unsigned)seed, res)) return api_error(rc) == 0;
  // the pairs' generators after their fills: one sweep through the seed's stream, in the order of the words taken
  out.assign(pairs.size(), PairTables());
  std::vector<size_t> order(mine.size());
  for (size_t j = 0; j < order.size(); j++) order[j] = j;
  std::sort(order.begin(), order.end(), [&](size_t a, size_t b) { return res.words[a] < res.words[b]; });
  std::mt19937 g0((unsigned)seed);
  BulkMt19937 bulk;
  if (!bulk.load(g0)) return false;
  unsigned long long at = 0;
  int handed_back = 0;
  for (size_t j : order) {
    PairTables& pt = out[todo[j]];
    bulk.skip(res.words[j] - at), at = res.words[j];
    if (!bulk.store(pt.rng)) return false;
    const double* const src = res.tables.data() + res.table_off[j];
    pt.set_blocks(res.nb[j], A, [src, A](int b) { return src + (size_t)b * 4 * A; });
    handed_back += res.handed_back[j];
  }
  std::cerr << in.S << " samples and " << in.M << " masks staged, " << mine.size() << " pairs walked and filled on the device ("
            << handed_back << " handed back to the host)" << std::endl;
  g_times.parse_mut = t1 - t0, g_times.table_fill = StageTimes::now() - t1;
  if (g_times.on)
    std::cerr << "Timing: samples fill: inputs " << t1 - t0 << " s, walks and fills " << g_times.table_fill << " s (device kernels "
              << res.kernel_s << " s, " << res.chunks << " chunk(s)); " << in.row_off.back() << " rows, " << in.S << " index arrays and "
              << in.M << " masks staged, " << 100 * *std::max_element(res.used.begin(), res.used.end()) << " uniforms uploaded" << std::endl;
  return true;
}

}  // namespace colate_drv

extern "C" {

int colate_fill_samples(int C, const long long* row_off, const colate_walk_row* rows, int S, const colate_walk_idx* idx, int M,
                        const unsigned long long* masks, int P, const colate_walk_pair* pairs, int num_bases_per_block, int A,
                        unsigned int seed, long long cap_blocks, int* out_nb, long long* out_used, double* out_tables,
                        unsigned long long* out_words, int* out_handed_back) {
  const colate_fs::FlatView f(C, row_off, rows, S, idx, M, masks, P, pairs, num_bases_per_block);
  return colate_fs::fill_call(true, f, A, seed, cap_blocks, out_nb, out_used, out_tables, out_words, out_handed_back, nullptr);
}

int colate_fill_samples_host(int C, const long long* row_off, const colate_walk_row* rows, int S, const colate_walk_idx* idx, int M,
                             const unsigned long long* masks, int P, const colate_walk_pair* pairs, int num_bases_per_block, int A,
                             unsigned int seed, long long cap_blocks, int* out_nb, long long* out_used, double* out_tables,
                             unsigned long long* out_words, int* out_handed_back, int* out_near_band) {
  const colate_fs::FlatView f(C, row_off, rows, S, idx, M, masks, P, pairs, num_bases_per_block);
  return colate_fs::fill_call(false, f, A, seed, cap_blocks, out_nb, out_used, out_tables, out_words, out_handed_back, out_near_band);
}

int colate_fill_samples_chunks(void) { return colate_fs::g_chunks; }
double colate_fill_samples_kernel_seconds(void) { return colate_fs::g_kernel_s; }

}  // extern "C"
