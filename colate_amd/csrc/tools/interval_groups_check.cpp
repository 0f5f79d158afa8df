// colate_amd/csrc/tools/interval_groups_check.cpp -- stand-alone run of the host side of colate_interval_fit_groups and of
// the many-pairs record collection of `Colate --mode mut_interval --pairs`:
//   * colate_interval_fit_groups_host (math 0 and 1) on G = 4 groups of 1, 3, 5 and 2 genome blocks -- one block empty,
//     records beyond the grid among them -- against colate_interval_cells_host -> colate_bootstrap_em_interval_batch_host
//     group by group, every bit; the same with a group without records in the middle;
//   * the argument checks: G < 1, a decreasing rec_off, a bad record, a negative block weight and epochs out of order are
//     COLATE_EINVAL, name the group, and leave every output alone;
//   * collect_interval_records_pairs over small synthetic inputs written here (two chromosomes of three genome blocks, two
//     targets, one reference; a pair listed twice): every pair's records, blocks and block count are those of
//     collect_interval_records for the pair alone, and the grouped host twin runs on them;
//   * plan_chunks, the rule by which the device form cuts the groups into chunks that share scratch: the cases the GPU tests
//     assume (a segment budget of 3 over 1,3,5,2,1 and 1,1,1,3,1 blocks; budget 0), a record budget, the cap of 65535 groups per
//     chunk, and random inputs against the rule's properties.
// For the host sanitizer build (`make asan`: bin/interval_groups_check_asan, linked with tools/no_device_stubs.cpp); prints
// "ok" and exits 0 when everything agrees.  Usage: interval_groups_check_asan DIR (an existing, writable directory).
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "colate_amd.h"
#include "interval_groups.h"
#include "cli_lists.h"
#include "walk_inputs.h"

namespace {

unsigned g_s = 4711;
unsigned next() { return (g_s = g_s * 1664525u + 1013904223u) >> 8; }

struct Groups {
  std::vector<long long> rec_off{0};
  std::vector<colate_interval_rec> recs;
  std::vector<int> block, nb;
  std::vector<double> bw;
  void add(int nb_g, int per_block, int empty_block, int B) {
    for (int k = 0; k < nb_g; k++)
      for (int i = 0; i < (k == empty_block ? 0 : per_block); i++) {
        colate_interval_rec r;
        r.begin = (float)(std::exp((next() % 900) / 100.0) * 3.0);
        r.end = r.begin * (1.0f + (next() % 250) / 100.0f);
        if (i % 11 == 0) r.begin = 0.0f;
        if (i % 17 == 0) r.end = r.begin;
        if (i % 29 == 0) r.end = 3e7f;  // beyond the grid
        r.w_sh = std::pow(10.0, (int)(next() % 5) - 2) * (1 + next() % 1000) / 1000.0 * (next() % 5 != 0);
        r.w_ns = std::pow(10.0, (int)(next() % 5) - 2) * (1 + next() % 1000) / 1000.0;
        recs.push_back(r), block.push_back(k);
      }
    rec_off.push_back((long long)recs.size());
    nb.push_back(nb_g);
    for (int b = 0; b < B; b++) {  // whole numbers that sum to nb_g, zeros among them
      std::vector<double> w((size_t)nb_g, 0.0);
      for (int k = 0; k < nb_g; k++) w[next() % (unsigned)nb_g] += 1.0;
      bw.insert(bw.end(), w.begin(), w.end());
    }
  }
  int G() const { return (int)nb.size(); }
};

struct Results {
  std::vector<int> R, iters, flags;
  std::vector<long long> dropped;
  std::vector<double> rates, ll;
  Results(int G, int B, int E, int fill = 0)
      : R((size_t)G, fill), iters((size_t)G * B, fill), flags((size_t)G * B, fill), dropped((size_t)G, fill), rates((size_t)G * B * E, fill),
        ll((size_t)G * B, fill) {}
  bool same(const Results& o) const {
    auto eq = [](const auto& a, const auto& b) { return a.size() == b.size() && std::memcmp(a.data(), b.data(), a.size() * sizeof(a[0])) == 0; };
    return eq(R, o.R) && eq(iters, o.iters) && eq(flags, o.flags) && eq(dropped, o.dropped) && eq(rates, o.rates) && eq(ll, o.ll);
  }
};

const int kMaxIter = 40, kMinIter = 10;

int grouped(const Groups& g, int B, int E, const double* ep, const double* init, int math, Results& out) {
  return colate_interval_fit_groups_host(g.G(), B, E, g.rec_off.data(), g.recs.data(), g.block.data(), g.nb.data(), g.bw.data(), ep, init,
                                         kMaxIter, kMinIter, COLATE_DEFAULT_REL_TOL, COLATE_DEFAULT_RATE_FLOOR, out.R.data(), out.dropped.data(),
                                         out.rates.data(), out.iters.data(), out.ll.data(), out.flags.data(), math);
}

// the two host calls group by group
int composed(const Groups& g, int B, int E, const double* ep, const double* init, int math, Results& out) {
  size_t w_off = 0;
  for (int i = 0; i < g.G(); i++) {
    const long long n = g.rec_off[(size_t)i + 1] - g.rec_off[(size_t)i];
    const int nb = g.nb[(size_t)i], cap = (int)std::min<long long>(COLATE_INTERVAL_MAX_ROWS, 2 * n);
    std::vector<int> kinds((size_t)cap);
    std::vector<double> a0((size_t)cap), a1((size_t)cap), tab((size_t)nb * cap);
    const int R = colate_interval_cells_host(n, g.recs.data() + g.rec_off[(size_t)i], g.block.data() + g.rec_off[(size_t)i], nb, cap, kinds.data(),
                                             a0.data(), a1.data(), tab.data(), &out.dropped[(size_t)i]);
    if (R < 0) return R;
    out.R[(size_t)i] = R;
    const size_t o = (size_t)i * B;
    if (R == 0) {
      for (int b = 0; b < B; b++) std::memcpy(&out.rates[(o + b) * E], init + (size_t)i * E, sizeof(double) * (size_t)E);
    } else if (int rc = colate_bootstrap_em_interval_batch_host(B, nb, R, E, kinds.data(), a0.data(), a1.data(), g.bw.data() + w_off, tab.data(),
                                                                ep + (size_t)i * E, init + (size_t)i * E, kMaxIter, kMinIter,
                                                                COLATE_DEFAULT_REL_TOL, COLATE_DEFAULT_RATE_FLOOR, &out.rates[o * E],
                                                                &out.iters[o], &out.ll[o], &out.flags[o], math))
      return rc;
    w_off += (size_t)B * nb;
  }
  return 0;
}

// ---- small synthetic inputs of `--mode mut`: P_chr<c>.mut, and .colate.in files of records (chrom, bp, anc, der, AAF, DAF)
void put_rec(FILE* f, const std::string& chrom, int bp, char anc, char der, int aaf, int daf) {
  const int n = (int)chrom.size();
  std::fwrite(&n, 4, 1, f), std::fwrite(chrom.data(), 1, chrom.size(), f), std::fwrite(&bp, 4, 1, f);
  std::fwrite(&anc, 1, 1, f), std::fwrite(&der, 1, 1, f), std::fwrite(&aaf, 4, 1, f), std::fwrite(&daf, 4, 1, f);
}
bool write_inputs(const std::string& dir, const std::vector<std::string>& chroms, int snps) {
  FILE* ta = std::fopen((dir + "/Ta.colate.in").c_str(), "wb");
  FILE* tb = std::fopen((dir + "/Tb.colate.in").c_str(), "wb");
  FILE* ra = std::fopen((dir + "/Ra.colate.in").c_str(), "wb");
  if (!ta || !tb || !ra) return false;
  const char bases[] = "ACGT";
  for (const std::string& c : chroms) {
    FILE* m = std::fopen((dir + "/P_chr" + c + ".mut").c_str(), "w");
    if (!m) return false;
    std::fprintf(m, "snp;pos_of_snp;dist;rs-id;tree_index;branch_indices;is_not_mapping;is_flipped;age_begin;age_end;"
                    "ancestral_allele/alternative_allele;upstream_allele;downstream_allele;\n");
    int bp = 1000;
    for (int i = 0; i < snps; i++) {
      bp += 1 + (int)(next() % 400000);  // about 200 kb apart: `snps` = 400 spans three blocks of 30 Mb
      const double begin = i % 13 == 0 ? 0.0 : std::exp((next() % 1000) / 100.0) * 2.0;
      const double end = (begin > 30.0 ? begin : 30.0) * (1.0 + (next() % 150) / 100.0);
      const char a = bases[next() % 4], d = bases[(std::strchr(bases, a) - bases + 1 + next() % 3) % 4];
      std::fprintf(m, "%d;%d;%d;rs%d;%d;%s;0;%d;%.6g;%.6g;%c/%c;%c;%c;\n", i, bp, 100, i, i / 10, next() % 25 ? "7" : "7 12", next() % 33 == 0,
                   begin, end, a, d, a, d);
      if (next() % 10) {
        const int daf = (int)(next() % 3);
        put_rec(ra, c, bp + (next() % 20 == 0), a, d, 2 - daf, daf);
      }
      for (FILE* t : {ta, tb})
        if (next() % 10) {
          const int n = (int)(next() % 5), daf = n ? (int)(next() % (unsigned)(n + 1)) : 0;
          put_rec(t, c, bp, a, d, n - daf, daf);
        }
    }
    std::fclose(m);
  }
  return std::fclose(ta) == 0 && std::fclose(tb) == 0 && std::fclose(ra) == 0;
}

// ---- plan_chunks
using Chunks = std::vector<std::pair<int, int>>;
const size_t kNoSegLimit = ~(size_t)0 / 2;
const long long kNoRecLimit = 0x7fffffffffffffffLL;

// `per_group` records in every group
std::vector<long long> even_rec_off(size_t G, long long per_group) {
  std::vector<long long> off(G + 1);
  for (size_t g = 0; g <= G; g++) off[g] = (long long)g * per_group;
  return off;
}
int expect_chunks(const char* what, const std::vector<int>& nb, long long per_group, size_t budget_segs, long long max_recs, const Chunks& want) {
  const std::vector<long long> off = even_rec_off(nb.size(), per_group);
  const Chunks got = colate_ic::plan_chunks((int)nb.size(), nb.data(), off.data(), budget_segs, max_recs);
  if (got == want) return 0;
  std::fprintf(stderr, "plan_chunks %s:", what);
  for (const auto& c : got) std::fprintf(stderr, " [%d, %d)", c.first, c.second);
  std::fprintf(stderr, ", expected %zu chunks\n", want.size());
  return 1;
}
// in order and without gaps over [0, G); a chunk of more than one group within both budgets and the cap
int check_partition(const Chunks& ch, const std::vector<int>& nb, const std::vector<long long>& off, size_t budget_segs, long long max_recs) {
  int at = 0, bad = 0;
  for (const auto& c : ch) {
    bad += c.first != at || c.second <= c.first;
    at = c.second;
    size_t segs = 0;
    for (int g = c.first; g < c.second && g < (int)nb.size(); g++) segs += (size_t)nb[(size_t)g];
    if (c.second - c.first > 1 && c.second <= (int)nb.size())
      bad += segs > std::max<size_t>(1, budget_segs) || off[(size_t)c.second] - off[(size_t)c.first] > max_recs || c.second - c.first > 65535;
  }
  return bad + (at != (int)nb.size());
}
int check_plan_chunks() {
  int bad = 0;
  const std::vector<int> nb_a = {1, 3, 5, 2, 1}, nb_c = {1, 1, 1, 3, 1};
  bad += expect_chunks("(a)", nb_a, 10, 3, kNoRecLimit, {{0, 1}, {1, 2}, {2, 3}, {3, 5}});
  bad += expect_chunks("(b)", nb_a, 10, 0, kNoRecLimit, {{0, 1}, {1, 2}, {2, 3}, {3, 4}, {4, 5}});
  bad += expect_chunks("(c)", nb_c, 10, 3, kNoRecLimit, {{0, 3}, {3, 4}, {4, 5}});
  bad += expect_chunks("(d)", nb_c, 15000, kNoSegLimit, (1 << 20) / 28, {{0, 2}, {2, 4}, {4, 5}});
  bad += expect_chunks("(e)", std::vector<int>(65536, 1), 0, kNoSegLimit, kNoRecLimit, {{0, 65535}, {65535, 65536}});
  for (int trial = 0; trial < 200; trial++) {  // (f)
    const size_t G = 1 + next() % 40;
    std::vector<int> nb(G);
    std::vector<long long> off(G + 1, (long long)(next() % 5));
    for (size_t g = 0; g < G; g++) nb[g] = 1 + (int)(next() % 9), off[g + 1] = off[g] + (next() % 4 ? (long long)(next() % 1000) : 0);
    const size_t budget_segs = next() % 4 ? next() % 30 : kNoSegLimit;
    const long long max_recs = next() % 4 ? (long long)(next() % 3000) : kNoRecLimit;
    const int b = check_partition(colate_ic::plan_chunks((int)G, nb.data(), off.data(), budget_segs, max_recs), nb, off, budget_segs, max_recs);
    if (b) std::fprintf(stderr, "plan_chunks (f), trial %d: %d violations\n", trial, b);
    bad += b;
  }
  return bad;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) {
    std::fprintf(stderr, "usage: %s DIR\n", argv[0]);
    return 2;
  }
  int bad = check_plan_chunks();
  const int B = 3;
  std::vector<double> ep1(COLATE_MAX_EPOCHS);
  int ep_null = 0;
  const int E = colate_epochs_from_bins("3,7,0.2", 0.0, 28.0, ep1.data(), COLATE_MAX_EPOCHS, &ep_null);
  if (E <= 0) return 1;

  // ---- the host twin against the two host calls, G = 4 and G = 5 with a group without records in the middle
  for (int with_empty = 0; with_empty < 2; with_empty++) {
    Groups g;
    g.add(1, 60, -1, B), g.add(3, 40, 1, B);
    if (with_empty) g.add(2, 0, -1, B);
    g.add(5, 30, -1, B), g.add(2, 50, -1, B);
    const int G = g.G();
    std::vector<double> ep, init;
    for (int i = 0; i < G; i++) {
      ep.insert(ep.end(), ep1.begin(), ep1.begin() + E);
      init.insert(init.end(), (size_t)E, COLATE_DEFAULT_INIT_RATE * (1 + i));
    }
    for (int math = 0; math < 2; math++) {
      Results got(G, B, E), want(G, B, E);
      const int rc = grouped(g, B, E, ep.data(), init.data(), math, got), rc2 = composed(g, B, E, ep.data(), init.data(), math, want);
      if (rc || rc2 || !got.same(want)) {
        std::fprintf(stderr, "G = %d, math %d: rc %d / %d (%s), results %s\n", G, math, rc, rc2, colate_last_error(), got.same(want) ? "equal" : "differ");
        bad++;
      }
      if (with_empty) bad += got.R[2] != 0 || got.iters[2 * B] != 0 || got.rates[(size_t)2 * B * E] != init[(size_t)2 * E];
    }
    if (with_empty) continue;
    // ---- refusals: COLATE_EINVAL, the group named, nothing written
    const Results mark(G, B, E, -7);
    auto refused = [&](const Groups& h, const std::vector<double>& e, const char* what) {
      Results out(G, B, E, -7);
      const int rc = grouped(h, B, E, e.data(), init.data(), 1, out);
      if (rc != COLATE_EINVAL || !std::strstr(colate_last_error(), what) || !out.same(mark)) {
        std::fprintf(stderr, "refusal `%s`: rc %d, message `%s`, outputs %s\n", what, rc, colate_last_error(), out.same(mark) ? "untouched" : "written");
        bad++;
      }
    };
    Groups h = g;
    h.rec_off[2] = h.rec_off[1] - 1;
    refused(h, ep, "rec_off decreases at group 1");
    h = g, h.recs[(size_t)h.rec_off[2] + 3].end = -1.0f;
    refused(h, ep, "group 2: record 3");
    h = g, h.block[(size_t)h.rec_off[1]] = 2;
    refused(h, ep, "group 1: record");
    h = g, h.bw[(size_t)B * 1 + 1] = -1.0;
    refused(h, ep, "group 1: block weight");
    h = g, h.nb[3] = 0;
    refused(h, ep, "group 3: bad sizes");
    std::vector<double> e2 = ep;
    std::swap(e2[(size_t)2 * E + 4], e2[(size_t)2 * E + 5]);
    refused(g, e2, "group 2: epochs must be non-decreasing");
    e2 = ep;
    for (int e = 0; e < E; e++) e2[(size_t)E + e] += 50.0;  // the rows of group 1 start at age 0
    refused(g, e2, "group 1: call 0: age_begin");
    Results out(G, B, E, -7);
    bad += colate_interval_fit_groups_host(0, B, E, g.rec_off.data(), g.recs.data(), g.block.data(), g.nb.data(), g.bw.data(), ep.data(), init.data(),
                                           kMaxIter, kMinIter, 1e-3, 0.0, out.R.data(), out.dropped.data(), out.rates.data(), out.iters.data(),
                                           out.ll.data(), out.flags.data(), 1) != COLATE_EINVAL || !out.same(mark);
    bad += colate_interval_fit_groups(G, B, E, g.rec_off.data(), g.recs.data(), g.block.data(), g.nb.data(), g.bw.data(), ep.data(), init.data(),
                                      kMaxIter, kMinIter, 1e-3, 0.0, out.R.data(), out.dropped.data(), out.rates.data(), out.iters.data(),
                                      out.ll.data(), out.flags.data()) != COLATE_ENODEVICE || !out.same(mark);
  }

  // ---- the many-pairs record collection against the single-pair one
  using namespace colate_drv;
  const std::string dir = argv[1];
  const std::vector<std::string> names = {"1", "2"};
  if (!write_inputs(dir, names, 400)) {
    std::fprintf(stderr, "cannot write the inputs under %s\n", dir.c_str());
    return 1;
  }
  std::vector<std::string> mut_files;
  for (const std::string& c : names) mut_files.push_back(dir + "/P_chr" + c + ".mut");
  std::vector<PairSpec> pairs(3);
  pairs[0].target = dir + "/Ta.colate.in", pairs[1].target = dir + "/Tb.colate.in", pairs[2].target = pairs[0].target;
  for (PairSpec& p : pairs) p.reference = dir + "/Ra.colate.in";
  std::vector<PairRecords> many;
  if (!collect_interval_records_pairs(names, mut_files, pairs, many) || many.size() != pairs.size()) return 1;
  Groups g;
  for (size_t p = 0; p < pairs.size(); p++) {
    std::vector<colate_interval_rec> recs;
    std::vector<int> blocks;
    int nb = 0;
    const bool ok = collect_interval_records(names, mut_files, pairs[p], recs, blocks, nb);
    const PairRecords& m = many[p];
    const bool same = ok && m.walked && nb == m.nb && recs.size() == m.recs.size() && blocks == m.blocks &&
                      (recs.empty() || std::memcmp(recs.data(), m.recs.data(), recs.size() * sizeof(recs[0])) == 0);
    if (!same || recs.size() < 50 || nb < 4) {
      std::fprintf(stderr, "pair %zu: %zu records in %d blocks alone, %zu in %d among many\n", p, recs.size(), nb, m.recs.size(), m.nb);
      bad++;
    }
    g.recs.insert(g.recs.end(), m.recs.begin(), m.recs.end()), g.block.insert(g.block.end(), m.blocks.begin(), m.blocks.end());
    g.rec_off.push_back((long long)g.recs.size()), g.nb.push_back(m.nb);
    std::mt19937 rng(5);
    g.bw.resize(g.bw.size() + (size_t)B * m.nb);
    if (colate_bootstrap_weights(&rng, B, m.nb, g.bw.data() + g.bw.size() - (size_t)B * m.nb)) return 1;
  }
  bad += many[0].recs.size() == many[1].recs.size() && std::memcmp(many[0].recs.data(), many[1].recs.data(), many[0].recs.size() * sizeof(colate_interval_rec)) == 0;
  {
    const int G = g.G();
    std::vector<double> ep, init((size_t)G * E, COLATE_DEFAULT_INIT_RATE);
    for (int i = 0; i < G; i++) ep.insert(ep.end(), ep1.begin(), ep1.begin() + E);
    Results got(G, B, E), want(G, B, E);
    const int rc = grouped(g, B, E, ep.data(), init.data(), 1, got), rc2 = composed(g, B, E, ep.data(), init.data(), 1, want);
    if (rc || rc2 || !got.same(want) || got.R[0] < 50) {
      std::fprintf(stderr, "pairs' records: rc %d / %d (%s), R %d\n", rc, rc2, colate_last_error(), got.R[0]);
      bad++;
    }
    bad += std::memcmp(&got.rates[0], &got.rates[(size_t)2 * B * E], sizeof(double) * (size_t)B * E) != 0;  // the pair listed twice
    std::printf("%d pairs, %lld records, rows %d %d %d\n", G, g.rec_off.back(), got.R[0], got.R[1], got.R[2]);
  }
  if (bad) {
    std::fprintf(stderr, "%d mismatches\n", bad);
    return 1;
  }
  std::printf("ok\n");
  return 0;
}
