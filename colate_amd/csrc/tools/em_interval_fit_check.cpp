// colate_amd/csrc/tools/em_interval_fit_check.cpp -- stand-alone run of the two host twins of colate_em_interval_batch
// (colate_em_interval_batch_host, math 0 and 1) over one fit of the size of tests/golden/l2_interval_fit: 23 epochs
// (--bins 3,7,0.2), 60 rows (points, intervals inside one epoch, intervals into the open last epoch, both kinds),
// 3 replicates with small integer weights and zeros.  For the host sanitizer build (`make asan`:
// bin/em_interval_fit_check_asan, linked with tools/no_device_stubs.cpp); exits 0 when both twins return finite
// rates and the same iteration counts, and a refused call leaves its outputs alone.
#include <cmath>
#include <cstdio>
#include <vector>

#include "colate_amd.h"

int main() {
  const int E = 23, R = 60, B = 3;
  std::vector<double> ep(E), init(E, COLATE_DEFAULT_INIT_RATE);
  ep[0] = 0.0;
  for (int e = 1; e < E - 1; e++) ep[e] = std::pow(10.0, 3.0 + 0.2 * (e - 1)) / 28.0;
  ep[E - 1] = 1e8 / 28.0;
  std::vector<int> kinds(R);
  std::vector<double> a0(R), a1(R), w((size_t)B * R);
  unsigned s = 12345;
  auto next = [&s] { return (s = s * 1664525u + 1013904223u) >> 8; };
  for (int r = 0; r < R; r++) {
    kinds[r] = r & 1;
    a0[r] = std::exp((next() % 85) / 5.0) / 10.0;
    a1[r] = (r % 3 == 0) ? a0[r] : a0[r] * (1.0 + (next() % 400) / 100.0);
    if (r % 7 == 3) a1[r] = ep[E - 1] * 1.5;  // into the open last epoch
    if (r % 11 == 5) a0[r] = 40.0, a1[r] = 41.0;  // inside one epoch
    for (int b = 0; b < B; b++) w[(size_t)b * R + r] = (double)(next() % 4);
  }
  int bad = 0;
  std::vector<int> iters[2];
  for (int math = 0; math < 2; math++) {
    std::vector<double> rates((size_t)B * E), ll(B);
    std::vector<int> flags(B);
    iters[math].assign(B, -1);
    const int rc = colate_em_interval_batch_host(B, R, E, kinds.data(), a0.data(), a1.data(), w.data(), ep.data(), init.data(),
                                                 400, 20, 1e-6, COLATE_DEFAULT_RATE_FLOOR, rates.data(), iters[math].data(),
                                                 ll.data(), flags.data(), math);
    if (rc != COLATE_OK) {
      std::fprintf(stderr, "math %d: rc %d: %s\n", math, rc, colate_last_error());
      return 1;
    }
    for (int b = 0; b < B; b++) {
      std::printf("math %d replicate %d: iterations %d, loglik %.17g, flags %d, rates", math, b, iters[math][b], ll[b], flags[b]);
      for (int e = 0; e < E; e++) {
        std::printf(" %a", rates[(size_t)b * E + e]);
        if (!std::isfinite(rates[(size_t)b * E + e])) bad++;
      }
      std::printf("\n");
      if (!std::isfinite(ll[b]) || (flags[b] & (COLATE_FLAG_NAN | COLATE_FLAG_NEG))) bad++;
    }
  }
  for (int b = 0; b < B; b++) bad += iters[0][b] != iters[1][b];
  // a refusal touches nothing
  std::vector<double> rates((size_t)B * E, -7.0), ll(B, -7.0);
  std::vector<int> it(B, -7), fl(B, -7);
  w[5] = -1.0;
  const int rc = colate_em_interval_batch_host(B, R, E, kinds.data(), a0.data(), a1.data(), w.data(), ep.data(), init.data(), 400,
                                               20, 1e-6, COLATE_DEFAULT_RATE_FLOOR, rates.data(), it.data(), ll.data(), fl.data(), 0);
  bad += rc != COLATE_EINVAL;
  for (double x : rates) bad += x != -7.0;
  for (int b = 0; b < B; b++) bad += ll[b] != -7.0 || it[b] != -7 || fl[b] != -7;
  std::printf("%s\n", bad ? "FAILED" : "ok");
  return bad ? 1 : 0;
}
