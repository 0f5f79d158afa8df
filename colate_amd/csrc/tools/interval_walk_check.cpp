// colate_amd/csrc/tools/interval_walk_check.cpp -- stand-alone run of the host twin of the pair walk (interval_walk.h)
// against the engine's walk of `Colate --mode mut_interval`:
//   * small synthetic inputs written here (two chromosomes of three genome blocks, two targets, two references, a mask
//     that removes the first third of every chromosome), read, decoded and indexed by the loader of the command line
//     (load_walk_inputs: load_inputs / build_walk_index);
//   * colate_interval_walk_host on those arrays -- through the view the command line hands over and through the C entry
//     point on back-to-back copies -- against collect_interval_records_pairs for every pair (unmasked, masked on either
//     side and on both, one pair twice, target = reference): records, blocks and nb, byte for byte;
//   * the refusals of the call by name, nothing written; the device form ends in COLATE_ENODEVICE in this build.
// For the host sanitizer build (`make asan`: bin/interval_walk_check_asan, linked with tools/no_device_stubs.cpp); prints
// "ok" and exits 0 when everything agrees.  Usage: interval_walk_check_asan DIR (an existing, writable directory).
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "colate_amd.h"
#include "interval_walk.h"
#include "cli_lists.h"
#include "walk_inputs.h"

namespace {

unsigned g_s = 1234;
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
      const double begin = i % 13 == 0 ? 0.0 : std::exp((next() % 1000) / 100.0) * 2.0;
      const double end = (begin > 30.0 ? begin : 30.0) * (1.0 + (next() % 150) / 100.0);
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
  const std::string dir = argv[1];
  const std::vector<std::string> names = {"1", "2"};
  if (!write_inputs(dir, names, 400)) {
    std::fprintf(stderr, "cannot write the inputs under %s\n", dir.c_str());
    return 1;
  }
  std::vector<std::string> mut_files, mask;
  for (const std::string& c : names) mut_files.push_back(dir + "/P_chr" + c + ".mut"), mask.push_back(dir + "/m_chr" + c + ".fa");
  auto file = [&dir](const char* s) { return dir + "/" + s + ".colate.in"; };
  // (target, reference, target masked, reference masked)
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

  // ---- the engine's walk, and the arrays of the pair walk through the same loader
  std::vector<PairRecords> want;
  if (!collect_interval_records_pairs(names, mut_files, pairs, want) || (int)want.size() != P) return 1;
  WalkInputs in;
  if (!load_walk_inputs(names, mut_files, pairs, in) || !in.indexed || in.S != 4 || in.M != 1) {
    std::fprintf(stderr, "the inputs were not indexed (%d samples, %d masks)\n", in.S, in.M);
    return 1;
  }
  colate_iw::View v;
  v.C = C, v.row_off = in.row_off.data(), v.rows = in.row_ptrs.data(), v.S = in.S, v.idx = in.idx_ptrs.data(), v.M = in.M;
  v.masks = in.mask_ptrs.data(), v.P = P, v.pairs = in.pairs.data(), v.nbpb = kIntervalBasesPerBlock;
  const long long n = in.row_off.back();
  long long total = 0;
  for (const PairRecords& pr : want) total += (long long)pr.recs.size();

  auto compare = [&](const char* what, const std::vector<long long>& rec_off, const std::vector<int>& nb,
                     const std::vector<colate_interval_rec>& recs, const std::vector<int>& block) {
    for (int p = 0; p < P; p++) {
      const PairRecords& w = want[(size_t)p];
      const long long k = rec_off[(size_t)p + 1] - rec_off[(size_t)p];
      const bool same = w.walked && nb[(size_t)p] == w.nb && k == (long long)w.recs.size() &&
                        (k == 0 || (std::memcmp(&recs[(size_t)rec_off[(size_t)p]], w.recs.data(), (size_t)k * sizeof(colate_interval_rec)) == 0 &&
                                    std::memcmp(&block[(size_t)rec_off[(size_t)p]], w.blocks.data(), (size_t)k * sizeof(int)) == 0));
      if (!same) {
        std::fprintf(stderr, "%s, pair %d: %lld records in %d blocks, the engine %zu in %d\n", what, p, k, nb[(size_t)p], w.recs.size(), w.nb);
        bad++;
      }
    }
  };

  std::vector<long long> rec_off((size_t)P + 1, -1);
  std::vector<int> nb((size_t)P, -1), block((size_t)total, -1);
  std::vector<colate_interval_rec> recs((size_t)total);
  if (int rc = colate_iw::walk_view_host(v, total, rec_off.data(), nb.data(), recs.data(), block.data())) {
    std::fprintf(stderr, "walk_view_host: %d (%s)\n", rc, colate_last_error());
    return 1;
  }
  compare("view", rec_off, nb, recs, block);
  bad += want[0].recs.size() < 50 || want[0].nb < 4 || want[1].recs.size() >= want[0].recs.size() + 100 || want[3].recs.empty();
  bad += std::memcmp(&recs[(size_t)rec_off[0]], &recs[(size_t)rec_off[4]], sizeof(colate_interval_rec) * want[0].recs.size()) != 0;  // the pair listed twice

  // ---- the C entry point on back-to-back copies
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
  auto flat = [&](const long long* row_off, const colate_walk_pair* prs, int nbpb, long long cap, const colate_walk_row* rows, std::vector<long long>& ro,
                  std::vector<int>& b, std::vector<colate_interval_rec>& r, std::vector<int>& blk, bool device = false) {
    return (device ? colate_interval_walk : colate_interval_walk_host)(C, row_off, rows, in.S, idx.data(), in.M, masks.data(), P, prs, nbpb, cap,
                                                                     ro.data(), b.data(), r.data(), blk.data());
  };
  {
    std::vector<long long> ro((size_t)P + 1, -1);
    std::vector<int> b((size_t)P, -1), blk((size_t)total, -1);
    std::vector<colate_interval_rec> r((size_t)total);
    if (int rc = flat(in.row_off.data(), in.pairs.data(), kIntervalBasesPerBlock, total, in.rows.data(), ro, b, r, blk)) {
      std::fprintf(stderr, "colate_interval_walk_host: %d (%s)\n", rc, colate_last_error());
      return 1;
    }
    compare("C entry point", ro, b, r, blk);
  }

  // ---- refusals: the code, the name, nothing written
  auto refused = [&](const char* what, int code, const long long* row_off, const colate_walk_pair* prs, int nbpb, long long cap,
                     const colate_walk_row* rows, bool device = false) {
    std::vector<long long> ro((size_t)P + 1, -7);
    std::vector<int> b((size_t)P, -7), blk((size_t)total, -7);
    std::vector<colate_interval_rec> r((size_t)total, colate_interval_rec{-7.f, -7.f, -7.0, -7.0});
    const int rc = flat(row_off, prs, nbpb, cap, rows, ro, b, r, blk, device);
    bool untouched = true;
    for (long long x : ro) untouched = untouched && x == -7;
    for (int x : b) untouched = untouched && x == -7;
    for (int x : blk) untouched = untouched && x == -7;
    for (const colate_interval_rec& x : r) untouched = untouched && x.w_sh == -7.0;
    if (rc != code || !std::strstr(colate_last_error(), what) || !untouched) {
      std::fprintf(stderr, "refusal `%s`: rc %d, message `%s`, outputs %s\n", what, rc, colate_last_error(), untouched ? "untouched" : "written");
      bad++;
    }
  };
  std::vector<colate_walk_pair> prs = in.pairs;
  prs[2].target = in.S;
  refused("pair 2: sample id out of range", COLATE_EINVAL, in.row_off.data(), prs.data(), kIntervalBasesPerBlock, total, in.rows.data());
  prs = in.pairs, prs[1].reference_mask = in.M;
  refused("pair 1: mask id out of range", COLATE_EINVAL, in.row_off.data(), prs.data(), kIntervalBasesPerBlock, total, in.rows.data());
  std::vector<long long> ro2 = in.row_off;
  ro2[1] = ro2[2] + 1;
  refused("row_off decreases at chromosome 1", COLATE_EINVAL, ro2.data(), in.pairs.data(), kIntervalBasesPerBlock, total, in.rows.data());
  refused("num_bases_per_block = 0", COLATE_EINVAL, in.row_off.data(), in.pairs.data(), 0, total, in.rows.data());
  std::vector<colate_walk_row> rows2 = in.rows;
  rows2.back().pos = 0x7fffffff - kIntervalBasesPerBlock + 1;
  refused("at or above 2^31 - num_bases_per_block", COLATE_EINVAL, in.row_off.data(), in.pairs.data(), kIntervalBasesPerBlock, total, rows2.data());
  refused("NULL pointer", COLATE_EINVAL, in.row_off.data(), nullptr, kIntervalBasesPerBlock, total, in.rows.data());
  refused("NULL pointer", COLATE_EINVAL, in.row_off.data(), in.pairs.data(), kIntervalBasesPerBlock, total, nullptr);
  refused("needed: ", COLATE_ELIMIT, in.row_off.data(), in.pairs.data(), kIntervalBasesPerBlock, total - 1, in.rows.data());
  refused("no device", COLATE_ENODEVICE, in.row_off.data(), in.pairs.data(), kIntervalBasesPerBlock, total, in.rows.data(), true);

  std::printf("%d pairs over %d samples, %lld rows, %lld records\n", P, in.S, n, total);
  if (bad) {
    std::fprintf(stderr, "%d mismatches\n", bad);
    return 1;
  }
  std::printf("ok\n");
  return 0;
}
