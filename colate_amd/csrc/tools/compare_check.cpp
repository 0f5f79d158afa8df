// colate_amd/csrc/tools/compare_check.cpp -- stand-alone run of the two host forms of `Colate --mode compare_tmp`
// (compare_tmp.h) against each other:
//   * small synthetic inputs written here (two chromosomes some 45 Mb long, four .colate.in files; rows at equal positions,
//     rows with a negative age_end, which only this mode searches, flipped and two-branch rows, which it does not), read,
//     decoded and indexed by the loader of the command line (load_walk_inputs with RowSet::compare_tmp);
//   * the cursor walk (compare_cursor_pairs) against compare_view_host on the loader's view and against
//     colate_compare_samples_host on back-to-back copies, every int of every pair, both orders of a pair among them;
//   * mismatch <= snps, and a pair and its swap alike;
//   * the refusals of the call by name, nothing written; the device form ends in COLATE_ENODEVICE in this build.
// For the host sanitizer build (`make asan`: bin/compare_check_asan, linked with tools/no_device_stubs.cpp); prints "ok" and
// exits 0 when everything agrees.  Usage: compare_check_asan DIR (an existing, writable directory).
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "colate_amd.h"
#include "compare_tmp.h"
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
    int bp = 5000;
    for (int i = 0; i < snps; i++) {
      bp += (int)(next() % 300000) * (next() % 12 != 0);  // about 150 kb apart, some rows at equal positions
      double begin = i % 13 == 0 ? 0.0 : std::exp((next() % 1000) / 100.0) * 2.0;
      double end = (begin > 30.0 ? begin : 30.0) * (1.0 + (next() % 150) / 100.0);
      if (i % 17 == 3) begin = -9.0, end = -2.0;  // (searched here, not by `--mode mut`)
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
  const std::string dir = argv[1];
  const std::vector<std::string> names = {"1", "2"};
  if (!write_inputs(dir, names, 300)) {
    std::fprintf(stderr, "cannot write the inputs under %s\n", dir.c_str());
    return 1;
  }
  std::vector<std::string> mut_files;
  for (const std::string& c : names) mut_files.push_back(dir + "/P_chr" + c + ".mut");
  auto file = [&dir](const char* s) { return dir + "/" + s + ".colate.in"; };
  const char* const list[][2] = {{"Ta", "Ra"}, {"Ra", "Ta"}, {"Tb", "Ra"}, {"Ta", "Rb"}, {"Tb", "Rb"}, {"Ra", "Ra"}, {"Ta", "Tb"}};
  std::vector<PairSpec> pairs;
  for (const auto& l : list) {
    PairSpec ps;
    ps.target = file(l[0]), ps.reference = file(l[1]);
    pairs.push_back(ps);
  }
  const int P = (int)pairs.size(), C = (int)names.size();

  WalkInputs in;
  if (!load_walk_inputs(names, mut_files, pairs, in, RowSet::compare_tmp) || !in.indexed || !in.files_ok || in.S != 4 || (int)in.compare.size() != C) {
    std::fprintf(stderr, "the inputs were not indexed (%d samples)\n", in.S);
    return 1;
  }
  std::vector<int> want_mm, want_n;
  if (!compare_cursor_pairs(in, names, pairs, want_mm, want_n)) return 1;
  std::vector<int> first, last;
  long long Wt = 0;
  for (const CompareChromosome& cc : in.compare) first.push_back(cc.first_pos), last.push_back(cc.last_pos), Wt += cc.windows;
  if (Wt < 2 * 4 || (long long)want_n.size() != P * Wt) {
    std::fprintf(stderr, "%lld windows\n", Wt);
    return 1;
  }

  auto compare = [&](const char* what, const std::vector<long long>& win_off, const std::vector<int>& mm, const std::vector<int>& n) {
    if (win_off[(size_t)C] != Wt || mm != want_mm || n != want_n) {
      std::fprintf(stderr, "%s: %lld windows (the cursor walk: %lld), counts %s\n", what, win_off[(size_t)C], Wt,
                   mm == want_mm && n == want_n ? "equal" : "differ");
      bad++;
    }
  };
  colate_cmp::View v;
  v.C = C, v.row_off = in.row_off.data(), v.rows = in.row_ptrs.data(), v.S = in.S, v.idx = in.idx_ptrs.data(), v.P = P, v.pairs = in.pairs.data();
  v.first_pos = first.data(), v.last_pos = last.data(), v.window = colate_cmp::kBinSize;
  const long long cap = P * Wt;
  {
    std::vector<long long> win_off((size_t)C + 1, -1);
    std::vector<int> mm((size_t)cap, -1), n((size_t)cap, -1);
    if (int rc = colate_cmp::compare_view_host(v, cap, win_off.data(), mm.data(), n.data())) {
      std::fprintf(stderr, "compare_view_host: %d (%s)\n", rc, colate_last_error());
      return 1;
    }
    compare("view", win_off, mm, n);
  }
  long long total = 0;
  for (long long w = 0; w < Wt; w++) {
    total += want_n[(size_t)w];
    bad += want_mm[(size_t)w] != want_mm[(size_t)(Wt + w)] || want_n[(size_t)w] != want_n[(size_t)(Wt + w)];  // (Ta, Ra) and (Ra, Ta)
  }
  for (size_t k = 0; k < want_n.size(); k++) bad += want_mm[k] > want_n[k] || want_mm[k] < 0;
  bad += total < 20;

  // ---- the C entry point on back-to-back copies
  const long long nrows = in.row_off.back();
  std::vector<colate_walk_idx> idx((size_t)in.S * nrows);
  for (int c = 0; c < C; c++) {
    const size_t nc = (size_t)(in.row_off[(size_t)c + 1] - in.row_off[(size_t)c]);
    for (int s = 0; s < in.S; s++) std::memcpy(&idx[(size_t)s * nrows + in.row_off[(size_t)c]], in.idx_ptrs[(size_t)s * C + c], nc * sizeof(colate_walk_idx));
  }
  auto flat = [&](const long long* row_off, const colate_walk_pair* prs, const int* fp, const int* lp, int window, long long room,
                  const colate_walk_row* rows, std::vector<long long>& wo, std::vector<int>& mm, std::vector<int>& n, bool device = false) {
    return (device ? colate_compare_samples : colate_compare_samples_host)(C, row_off, rows, in.S, idx.data(), P, prs, fp, lp, window, room, wo.data(),
                                                                          mm.data(), n.data());
  };
  {
    std::vector<long long> wo((size_t)C + 1, -1);
    std::vector<int> mm((size_t)cap, -1), n((size_t)cap, -1);
    if (int rc = flat(in.row_off.data(), in.pairs.data(), first.data(), last.data(), colate_cmp::kBinSize, cap, in.rows.data(), wo, mm, n)) {
      std::fprintf(stderr, "colate_compare_samples_host: %d (%s)\n", rc, colate_last_error());
      return 1;
    }
    compare("C entry point", wo, mm, n);
  }

  // ---- refusals: the code, the name, nothing written
  auto refused = [&](const char* what, int code, const long long* row_off, const colate_walk_pair* prs, const int* fp, const int* lp, int window,
                     long long room, const colate_walk_row* rows, bool device = false) {
    std::vector<long long> wo((size_t)C + 1, -7);
    std::vector<int> mm((size_t)cap, -7), n((size_t)cap, -7);
    const int rc = flat(row_off, prs, fp, lp, window, room, rows, wo, mm, n, device);
    bool untouched = true;
    for (long long x : wo) untouched = untouched && x == -7;
    for (int x : mm) untouched = untouched && x == -7;
    for (int x : n) untouched = untouched && x == -7;
    if (rc != code || !std::strstr(colate_last_error(), what) || !untouched) {
      std::fprintf(stderr, "refusal `%s`: rc %d, message `%s`, outputs %s\n", what, rc, colate_last_error(), untouched ? "untouched" : "written");
      bad++;
    }
  };
  const int B = colate_cmp::kBinSize;
  std::vector<colate_walk_pair> prs = in.pairs;
  prs[2].target = in.S;
  refused("pair 2: sample id out of range", COLATE_EINVAL, in.row_off.data(), prs.data(), first.data(), last.data(), B, cap, in.rows.data());
  prs = in.pairs, prs[1].reference_mask = 0;
  refused("pair 1: compare_tmp takes no masks", COLATE_EINVAL, in.row_off.data(), prs.data(), first.data(), last.data(), B, cap, in.rows.data());
  std::vector<long long> ro2 = in.row_off;
  ro2[1] = ro2[2] + 1;
  refused("row_off decreases at chromosome 1", COLATE_EINVAL, ro2.data(), in.pairs.data(), first.data(), last.data(), B, cap, in.rows.data());
  refused("window = 0", COLATE_EINVAL, in.row_off.data(), in.pairs.data(), first.data(), last.data(), 0, cap, in.rows.data());
  std::vector<int> f2 = first, l2 = last;
  f2[1] = in.rows[(size_t)in.row_off[1]].pos + 1;
  refused("chromosome 1: first_pos", COLATE_EINVAL, in.row_off.data(), in.pairs.data(), f2.data(), last.data(), B, cap, in.rows.data());
  l2[0] = in.rows[(size_t)in.row_off[1] - 1].pos - 1;
  refused("chromosome 0: last_pos", COLATE_EINVAL, in.row_off.data(), in.pairs.data(), first.data(), l2.data(), B, cap, in.rows.data());
  refused("NULL pointer", COLATE_EINVAL, in.row_off.data(), nullptr, first.data(), last.data(), B, cap, in.rows.data());
  refused("NULL pointer", COLATE_EINVAL, in.row_off.data(), in.pairs.data(), nullptr, last.data(), B, cap, in.rows.data());
  refused("NULL pointer", COLATE_EINVAL, in.row_off.data(), in.pairs.data(), first.data(), last.data(), B, cap, nullptr);
  refused("needed: ", COLATE_ELIMIT, in.row_off.data(), in.pairs.data(), first.data(), last.data(), B, cap - 1, in.rows.data());
  refused("no device", COLATE_ENODEVICE, in.row_off.data(), in.pairs.data(), first.data(), last.data(), B, cap, in.rows.data(), true);

  std::printf("%d pairs over %d samples, %lld rows, %lld windows, %lld counted rows in pair 0\n", P, in.S, nrows, Wt, total);
  if (bad) {
    std::fprintf(stderr, "%d mismatches\n", bad);
    return 1;
  }
  std::printf("ok\n");
  return 0;
}
