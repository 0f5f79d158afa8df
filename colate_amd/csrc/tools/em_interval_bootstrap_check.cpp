// colate_amd/csrc/tools/em_interval_bootstrap_check.cpp -- stand-alone run of the host side of
// colate_bootstrap_em_interval_batch: the rows-file parser of `Colate --mode mut_interval` (read_interval_rows) on a file
// it writes into the directory given as its argument (comments, a blank line, non-contiguous block ids, a repeated cell,
// both kinds, a point row, an interval into the open last epoch) and on malformed files, colate_bootstrap_rows_host,
// and colate_bootstrap_em_interval_batch_host (math 0 and 1) against colate_em_interval_batch_host on those sums.  For
// the host sanitizer build (`make asan`: bin/em_interval_bootstrap_check_asan, linked with tools/no_device_stubs.cpp);
// exits 0 when everything agrees bit for bit and every refusal leaves its outputs alone.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <random>
#include <string>
#include <vector>

#include "colate_amd.h"
#include "mut_interval.h"

using colate_drv::IntervalRows;
using colate_drv::read_interval_rows;

static int bad = 0;
#define EXPECT(cond)                                                  \
  do {                                                                \
    if (!(cond)) {                                                    \
      std::fprintf(stderr, "line %d: %s is false\n", __LINE__, #cond); \
      bad++;                                                          \
    }                                                                 \
  } while (0)

static void write_file(const std::string& path, const std::string& text) {
  std::ofstream os(path);
  os << text;
}

int main(int argc, char** argv) {
  if (argc < 2) {
    std::fprintf(stderr, "usage: %s DIRECTORY\n", argv[0]);
    return 2;
  }
  const std::string dir = argv[1];
  const int E = 23;
  std::vector<double> ep(E), init(E, COLATE_DEFAULT_INIT_RATE);
  int ep_null = 0;
  EXPECT(colate_epochs_from_bins("3,7,0.2", 0.0, 28.0, ep.data(), E, &ep_null) == E);

  // ---- the parser
  const std::string rows_path = dir + "/rows.txt";
  write_file(rows_path,
             "# block kind age_begin age_end weight\n"
             "40 shared 100 2500.5 2\n"
             "7 notshared 30 30 1.5\n"
             "\n"
             "40 notshared 30 30 4\n"
             "1000 shared 5e3 1e7 1\n"
             "7 shared 100 2500.5 3\n"
             "40 shared 1e2 2500.5 0.25\n"
             "1000 notshared 12.5 700 0\n");
  IntervalRows rows;
  std::string err;
  EXPECT(read_interval_rows(rows_path, ep[0], rows, err));
  EXPECT(rows.nb == 3 && rows.R == 4);
  if (rows.nb == 3 && rows.R == 4) {
    EXPECT(rows.block_ids[0] == 7 && rows.block_ids[1] == 40 && rows.block_ids[2] == 1000);
    EXPECT(rows.kinds[0] == 0 && rows.kinds[1] == 1 && rows.kinds[2] == 0 && rows.kinds[3] == 1);
    EXPECT(rows.age_begin[0] == 100 && rows.age_end[0] == 2500.5 && rows.age_begin[1] == rows.age_end[1]);
    EXPECT(rows.age_end[2] == 1e7 && rows.age_end[2] > ep[E - 1]);
    const double want[12] = {3, 1.5, 0, 0, 2.25, 4, 0, 0, 0, 0, 1, 0};
    EXPECT(std::memcmp(rows.tables.data(), want, sizeof(want)) == 0);
  }
  const char* malformed[] = {"7 shared 1 2\n", "7 both 1 2 1\n", "-7 shared 1 2 1\n", "7 shared 3 2 1\n", "7 shared 1 inf 1\n",
                             "7 shared 1 2 -1\n", "7 shared 1 2 nan\n", "7 shared x 2 1\n", "7 shared -1 2 1\n", "7.5 shared 1 2 1\n"};
  for (const char* m : malformed) {
    write_file(dir + "/bad.txt", std::string("# header\n7 shared 1 2 1\n") + m);
    IntervalRows r;
    err.clear();
    EXPECT(!read_interval_rows(dir + "/bad.txt", ep[0], r, err));
    EXPECT(err.find("line 3") != std::string::npos);
  }
  write_file(dir + "/empty.txt", "# nothing\n\n");
  EXPECT(!read_interval_rows(dir + "/empty.txt", ep[0], rows, err));
  EXPECT(!read_interval_rows(dir + "/missing.txt", ep[0], rows, err));
  EXPECT(read_interval_rows(rows_path, ep[0], rows, err));

  // ---- the weighted block sums and the fit behind them
  const int B = 4, nb = rows.nb, R = rows.R;
  std::mt19937 rng(5);
  std::vector<double> bw((size_t)B * nb), W((size_t)B * R, -7.0);
  EXPECT(colate_bootstrap_weights(&rng, B, nb, bw.data()) == COLATE_OK);
  EXPECT(colate_bootstrap_rows_host(B, nb, R, bw.data(), rows.tables.data(), W.data()) == COLATE_OK);
  for (int b = 0; b < B; b++)
    for (int r = 0; r < R; r++) {
      double acc = 0.0;
      for (int k = 0; k < nb; k++) {
        const double p = bw[(size_t)b * nb + k] * rows.tables[(size_t)k * R + r];
        acc = acc + p;
      }
      EXPECT(std::memcmp(&acc, &W[(size_t)b * R + r], sizeof(double)) == 0);
    }
  for (int math = 0; math < 2; math++) {
    std::vector<double> r1((size_t)B * E), r2((size_t)B * E), l1(B), l2(B);
    std::vector<int> i1(B), i2(B), f1(B), f2(B);
    EXPECT(colate_bootstrap_em_interval_batch_host(B, nb, R, E, rows.kinds.data(), rows.age_begin.data(), rows.age_end.data(),
                                                   bw.data(), rows.tables.data(), ep.data(), init.data(), 60, 20, 1e-6,
                                                   COLATE_DEFAULT_RATE_FLOOR, r1.data(), i1.data(), l1.data(), f1.data(),
                                                   math) == COLATE_OK);
    EXPECT(colate_em_interval_batch_host(B, R, E, rows.kinds.data(), rows.age_begin.data(), rows.age_end.data(), W.data(),
                                         ep.data(), init.data(), 60, 20, 1e-6, COLATE_DEFAULT_RATE_FLOOR, r2.data(), i2.data(),
                                         l2.data(), f2.data(), math) == COLATE_OK);
    EXPECT(std::memcmp(r1.data(), r2.data(), r1.size() * sizeof(double)) == 0);
    EXPECT(std::memcmp(l1.data(), l2.data(), l1.size() * sizeof(double)) == 0);
    EXPECT(i1 == i2 && f1 == f2);
    for (int b = 0; b < B; b++) std::printf("math %d replicate %d: iterations %d, loglik %.17g, flags %d\n", math, b, i1[b], l1[b], f1[b]);
  }
  // refusals touch nothing: a negative block weight, an overflowing sum, no block
  std::vector<double> rates((size_t)B * E, -7.0), ll(B, -7.0);
  std::vector<int> it(B, -7), fl(B, -7);
  auto refused = [&](int nb_, const std::vector<double>& bw_, const std::vector<double>& tab_) {
    const int rc = colate_bootstrap_em_interval_batch_host(B, nb_, R, E, rows.kinds.data(), rows.age_begin.data(),
                                                           rows.age_end.data(), bw_.data(), tab_.data(), ep.data(), init.data(), 60,
                                                           20, 1e-6, COLATE_DEFAULT_RATE_FLOOR, rates.data(), it.data(), ll.data(),
                                                           fl.data(), 1);
    EXPECT(rc == COLATE_EINVAL);
    for (double x : rates) EXPECT(x == -7.0);
    for (int b = 0; b < B; b++) EXPECT(ll[b] == -7.0 && it[b] == -7 && fl[b] == -7);
  };
  std::vector<double> bw_neg = bw, tab_big = rows.tables, bw_big = bw;
  bw_neg[1] = -1.0;
  refused(nb, bw_neg, rows.tables);
  tab_big[0] = tab_big[R] = 1.5e308, bw_big[0] = bw_big[1] = 1.0;
  refused(nb, bw_big, tab_big);
  refused(0, bw, rows.tables);
  std::vector<double> W2((size_t)B * R, -7.0);
  EXPECT(colate_bootstrap_rows_host(B, nb, R, bw_big.data(), tab_big.data(), W2.data()) == COLATE_EINVAL);
  for (double x : W2) EXPECT(x == -7.0);

  std::printf("%s\n", bad ? "FAILED" : "ok");
  return bad ? 1 : 0;
}
