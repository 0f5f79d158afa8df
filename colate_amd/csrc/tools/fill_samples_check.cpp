// colate_amd/csrc/tools/fill_samples_check.cpp -- stand-alone run of the host twin of the table fill over walk indices
// (fill_samples.h) against the engine's fill of `Colate --mode mut --pairs`:
//   * small synthetic inputs written here (two chromosomes of three genome blocks, two targets, two references, a mask that
//     removes the first third of every chromosome; every 13th row on the F path, some of them ending beyond the age grid, and
//     every 37th row a non-F row whose ages run from inside the grid to beyond it, so that its draws are repeated), read, decoded
//     and indexed by the loader of the command line (load_walk_inputs);
//   * fill_view_host on those arrays -- and the C entry point on back-to-back copies -- against fill_pairs for every pair
//     (unmasked, masked on either side and on both, one pair twice, target = reference): nb, the four raw tables of every
//     block and the generator at the end of the fill (a std::mt19937 on the seed after discard(words)), byte for byte;
//   * the refusals the call adds; the device form ends in COLATE_ENODEVICE in this build.
// For the host sanitizer build (`make asan`: bin/fill_samples_check_asan, linked with tools/no_device_stubs.cpp); prints "ok"
// and exits 0 when everything agrees.  Usage: fill_samples_check_asan DIR (an existing, writable directory).
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "colate_amd.h"
#include "fill_samples.h"
#include "interval_walk.h"
#include "cli_lists.h"
#include "walk_inputs.h"

namespace {

unsigned g_s = 4321;
unsigned next() { return (g_s = g_s * 1664525u + 1013904223u) >> 8; }

void put_rec(FILE* f, const std::string& chrom, int bp, char anc, char der, int aaf, int daf) {
  const int n = (int)chrom.size();
  std::fwrite(&n, 4, 1, f), std::fwrite(chrom.data(), 1, chrom.size(), f), std::fwrite(&bp, 4, 1, f);
  std::fwrite(&anc, 1, 1, f), std::fwrite(&der, 1, 1, f), std::fwrite(&aaf, 4, 1, f), std::fwrite(&daf, 4, 1, f);
}

// P_chr<c>.mut, four .colate.in files and m_chr<c>.fa (every position below 30 Mb removed)
bool write_inputs(const std::string& dir, const std::vector<std::string>& chroms, int snps) {
  const char* const files[4] = {"Ta", "Tb", "Ra", "Rb"};
  FILE* f[4];
  for (int k = 0; k < 4; k++)
    if (!(f[k] = std::fopen((dir + "/" + files[k] + ".colate.in").c_str(), "wb"))) return false;
  const char bases[] = "ACGT";
  for (const std::string& c : chroms) {
    FILE* m = std::fopen((dir + "/P_chr" + c + ".mut").c_str(), "w");
    if (!m) return false;
    std::fprintf(m, "snp;pos_of_snp;dist;rs-id;tree_index;branch_indices;is_not_mapping;is_flipped;age_begin;age_end;"
                    "ancestral_allele/alternative_allele;upstream_allele;downstream_allele;\n");
    int bp = 1000;
    for (int i = 0; i < snps; i++) {
      bp += (int)(next() % 400000) * (next() % 12 != 0);  // about 200 kb apart, some rows at equal positions
      double begin = i % 13 == 0 ? 0.0 : std::exp((next() % 1000) / 100.0) * 2.0;
      double end = (begin > 30.0 ? begin : 30.0) * (1.0 + (next() % 150) / 100.0);
      if (i % 39 == 0) end = 3e7;                   // an F row ending beyond the grid
      if (i % 37 == 5) begin = 5e6, end = 2e7;      // a non-F row pushed beyond the grid: draws are repeated
      const char a = bases[next() % 4], d = bases[(std::strchr(bases, a) - bases + 1 + next() % 3) % 4];
      std::fprintf(m, "%d;%d;%d;rs%d;%d;%s;0;%d;%.6g;%.6g;%c/%c;%c;%c;\n", i, bp, 100, i, i / 10, next() % 25 ? "7" : "7 12", next() % 33 == 0,
                   begin, end, a, d, a, d);
      for (int k = 0; k < 4; k++)
        if (next() % 10) {
          const int n = k < 2 ? (int)(next() % 5) : 2, daf = n ? (int)(next() % (unsigned)(n + 1)) : 0;
          put_rec(f[k], c, bp, next() % 30 ? a : d, d, n - daf, daf);
        }
    }
    std::fclose(m);
    FILE* fa = std::fopen((dir + "/m_chr" + c + ".fa").c_str(), "w");
    if (!fa) return false;
    std::fputs(">mask\n", fa);
    const std::string line(60, 'N');
    for (int k = 0; k < 30000000 / 60; k++) std::fputs(line.c_str(), fa), std::fputc('\n', fa);
    std::fclose(fa);
  }
  bool ok = true;
  for (int k = 0; k < 4; k++) ok = std::fclose(f[k]) == 0 && ok;
  return ok;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) {
    std::fprintf(stderr, "usage: %s DIR\n", argv[0]);
    return 2;
  }
  using namespace colate_drv;
  int bad = 0;
  const int A = 185, seed = 17;
  const std::string dir = argv[1];
  const std::vector<std::string> names = {"1", "2"};
  if (!write_inputs(dir, names, 400)) {
    std::fprintf(stderr, "cannot write the inputs under %s\n", dir.c_str());
    return 1;
  }
  std::vector<std::string> mut_files, mask;
  for (const std::string& c : names) mut_files.push_back(dir + "/P_chr" + c + ".mut"), mask.push_back(dir + "/m_chr" + c + ".fa");
  auto file = [&dir](const char* s) { return dir + "/" + s + ".colate.in"; };
  const struct {
    const char *t, *r;
    bool tm, rm;
  } list[] = {{"Ta", "Ra", false, false}, {"Tb", "Ra", true, false}, {"Ta", "Rb", false, true}, {"Tb", "Rb", true, true},
              {"Ta", "Ra", false, false}, {"Ra", "Ra", false, false}, {"Ra", "Tb", false, false}};
  std::vector<PairSpec> pairs;
  for (const auto& l : list) {
    PairSpec ps;
    ps.target = file(l.t), ps.reference = file(l.r);
    if (l.tm) ps.target_masks = mask;
    if (l.rm) ps.ref_masks = mask;
    pairs.push_back(ps);
  }
  const int P = (int)pairs.size(), C = (int)names.size();

  // ---- the engine's fill, and the twin on the arrays of the same loader
  std::vector<size_t> todo;
  for (int p = 0; p < P; p++) todo.push_back((size_t)p);
  std::vector<PairTables> want;
  if (!fill_pairs(Options(), names, mut_files, pairs, todo, seed, A, want) || (int)want.size() != P) return 1;
  WalkInputs in;
  if (!load_walk_inputs(names, mut_files, pairs, in) || !in.indexed || in.S != 4 || in.M != 1) {
    std::fprintf(stderr, "the inputs were not indexed (%d samples, %d masks)\n", in.S, in.M);
    return 1;
  }
  colate_iw::View v;
  v.C = C, v.row_off = in.row_off.data(), v.rows = in.row_ptrs.data(), v.S = in.S, v.idx = in.idx_ptrs.data(), v.M = in.M;
  v.masks = in.mask_ptrs.data(), v.P = P, v.pairs = in.pairs.data(), v.nbpb = kIntervalBasesPerBlock;

  auto compare = [&](const char* what, int p, int nb, const double* tab, unsigned long long words) {
    const PairTables& w = want[(size_t)p];
    bool same = nb == w.nb && nb >= 1;
    const std::vector<double>* const t[4] = {&w.sh, &w.ns, &w.she, &w.nse};
    for (int b = 0; same && b < nb; b++)
      for (int k = 0; k < 4; k++) same = same && std::memcmp(tab + ((size_t)b * 4 + k) * A, t[k]->data() + (size_t)b * A, sizeof(double) * A) == 0;
    std::mt19937 g((unsigned)seed);
    g.discard(words);
    if (!same || !(g == w.rng)) {
      std::fprintf(stderr, "%s, pair %d: %d blocks (the engine %d), tables %s, generator %s\n", what, p, nb, w.nb, same ? "equal" : "differ",
                   g == w.rng ? "equal" : "differs");
      bad++;
    }
  };

  colate_fs::Result res;
  if (int rc = colate_fs::fill_view_host(v, A, (unsigned)seed, res)) {
    std::fprintf(stderr, "fill_view_host: %d (%s)\n", rc, colate_last_error());
    return 1;
  }
  long long blocks = 0, used = 0;
  int redrawn = 0;
  for (int p = 0; p < P; p++) {
    compare("view", p, res.nb[(size_t)p], res.tables.data() + res.table_off[(size_t)p], res.words[(size_t)p]);
    blocks += res.nb[(size_t)p], used += res.used[(size_t)p];
    redrawn += res.words[(size_t)p] > 200ull * (unsigned long long)res.used[(size_t)p];
    bad += res.handed_back[(size_t)p] != 0;
    bad += res.near_band[(size_t)p] != (res.words[(size_t)p] > 200ull * (unsigned long long)res.used[(size_t)p]);  // (no draw this small run makes lies in a band)
  }
  bad += redrawn < 3 || res.used[0] < 50 || res.nb[0] < 4;  // the inputs are what they are meant to be
  bad += std::memcmp(res.tables.data() + res.table_off[0], res.tables.data() + res.table_off[4], sizeof(double) * (size_t)res.nb[0] * 4 * A) != 0;

  // ---- the C entry point on back-to-back copies
  const long long n = in.row_off.back();
  std::vector<long long> word_off((size_t)C + 1);
  const long long words = colate_iw::mask_words(C, in.row_off.data(), word_off.data());
  std::vector<colate_walk_idx> idx((size_t)in.S * n);
  std::vector<unsigned long long> masks((size_t)in.M * words);
  for (int c = 0; c < C; c++) {
    const size_t nc = (size_t)(in.row_off[(size_t)c + 1] - in.row_off[(size_t)c]);
    for (int s = 0; s < in.S; s++) std::memcpy(&idx[(size_t)s * n + in.row_off[(size_t)c]], in.idx_ptrs[(size_t)s * C + c], nc * sizeof(colate_walk_idx));
    for (int m = 0; m < in.M; m++)
      std::memcpy(&masks[(size_t)m * words + word_off[(size_t)c]], in.mask_ptrs[(size_t)m * C + c], (size_t)(word_off[(size_t)c + 1] - word_off[(size_t)c]) * 8);
  }
  struct Out {
    std::vector<int> nb, handed, near;
    std::vector<long long> used;
    std::vector<double> tables;
    std::vector<unsigned long long> words;
    Out(int P, long long blocks, int A) : nb((size_t)P, -7), handed((size_t)P, -7), near((size_t)P, -7), used((size_t)P, -7), tables((size_t)blocks * 4 * A, -7.0), words((size_t)P, 7) {}
    bool untouched() const {
      bool u = true;
      for (int x : nb) u = u && x == -7;
      for (double x : tables) u = u && x == -7.0;
      for (unsigned long long x : words) u = u && x == 7;
      return u;
    }
  };
  auto call = [&](Out& o, int a, long long cap, const colate_walk_pair* prs, bool device = false) {
    return device ? colate_fill_samples(C, in.row_off.data(), in.rows.data(), in.S, idx.data(), in.M, masks.data(), P, prs, kIntervalBasesPerBlock, a,
                                        (unsigned)seed, cap, o.nb.data(), o.used.data(), o.tables.data(), o.words.data(), o.handed.data())
                  : colate_fill_samples_host(C, in.row_off.data(), in.rows.data(), in.S, idx.data(), in.M, masks.data(), P, prs,
                                             kIntervalBasesPerBlock, a, (unsigned)seed, cap, o.nb.data(), o.used.data(), o.tables.data(),
                                             o.words.data(), o.handed.data(), o.near.data());
  };
  {
    Out o(P, blocks, A);
    if (int rc = call(o, A, blocks, in.pairs.data())) {
      std::fprintf(stderr, "colate_fill_samples_host: %d (%s)\n", rc, colate_last_error());
      return 1;
    }
    size_t at = 0;
    for (int p = 0; p < P; p++) compare("C entry point", p, o.nb[(size_t)p], o.tables.data() + at, o.words[(size_t)p]), at += (size_t)o.nb[(size_t)p] * 4 * A;
  }
  auto refused = [&](const char* what, int code, int a, long long cap, const colate_walk_pair* prs, bool device = false) {
    Out o(P, blocks, A);
    const int rc = call(o, a, cap, prs, device);
    if (rc != code || !std::strstr(colate_last_error(), what) || !o.untouched()) {
      std::fprintf(stderr, "refusal `%s`: rc %d, message `%s`, outputs %s\n", what, rc, colate_last_error(), o.untouched() ? "untouched" : "written");
      bad++;
    }
  };
  refused("the fill takes the 185 bins", COLATE_EINVAL, 184, blocks, in.pairs.data());
  refused("the fill takes the 185 bins", COLATE_EINVAL, 256, blocks, in.pairs.data());
  refused("needed: ", COLATE_ELIMIT, A, blocks - 1, in.pairs.data());
  refused("NULL pointer", COLATE_EINVAL, A, blocks, nullptr);
  std::vector<colate_walk_pair> prs = in.pairs;
  prs[2].target = in.S;
  refused("pair 2: sample id out of range", COLATE_EINVAL, A, blocks, prs.data());
  refused("no device", COLATE_ENODEVICE, A, blocks, in.pairs.data(), true);

  std::printf("%d pairs over %d samples, %lld rows, %lld used rows in %lld blocks, %d pairs with repeated draws\n", P, in.S, n, used, blocks, redrawn);
  if (bad) {
    std::fprintf(stderr, "%d mismatches\n", bad);
    return 1;
  }
  std::printf("ok\n");
  return 0;
}
