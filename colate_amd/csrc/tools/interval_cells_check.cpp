// colate_amd/csrc/tools/interval_cells_check.cpp -- stand-alone run of colate_interval_bin_thresholds and
// colate_interval_cells_host (the host twin of interval_cells_kernel.hip): the threshold table against the library
// expression at every step and its two neighbouring floats, and the twin over scripted records -- 3 genome blocks with the
// middle one empty, weights of mixed magnitude, records in one cell, a record from age 0, a point record, records beyond the
// age grid, exactly as many rows as there is room for -- against a plain ordered loop over a std::map, every bit.  For the
// host sanitizer build (`make asan`: bin/interval_cells_check_asan, linked with tools/no_device_stubs.cpp); prints "ok" and
// exits 0 when everything agrees and a refused call leaves its outputs alone.
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <tuple>
#include <vector>

#include "colate_amd.h"
#include "age_bins.hpp"

static int bin_libm(float x) { return colate_drv::age_bin_index((double)x, 10.0); }
static int bin_table(const float* T, float x) {
  int n = 0;
  for (int k = 0; k < COLATE_INTERVAL_BINS; k++) n += T[k] <= x;
  return n;
}

int main() {
  int bad = 0;
  float T[COLATE_INTERVAL_BINS];
  if (int rc = colate_interval_bin_thresholds(T)) {
    std::fprintf(stderr, "thresholds: rc %d: %s\n", rc, colate_last_error());
    return 1;
  }
  for (int n = 1; n <= COLATE_INTERVAL_BINS; n++) {
    const float t = T[n - 1];
    bad += bin_libm(t) != n || bin_libm(std::nextafterf(t, 0.0f)) != n - 1 || bin_libm(std::nextafterf(t, INFINITY)) < n;
    bad += n > 1 && !(T[n - 2] < t);
  }
  if (bad) std::fprintf(stderr, "thresholds: %d mismatches\n", bad);

  unsigned s = 2024;
  auto next = [&s] { return (s = s * 1664525u + 1013904223u) >> 8; };
  const int nb = 3;
  std::vector<colate_interval_rec> recs;
  std::vector<int> block;
  for (int k = 0; k < nb; k += 2)
    for (int i = 0; i < 700; i++) {
      colate_interval_rec r;
      r.begin = (float)(std::exp((next() % 1500) / 100.0) / 10.0);
      r.end = r.begin * (1.0f + (next() % 300) / 100.0f);
      if (i % 9 == 0) r.begin = 0.0f;              // the reference's F path
      if (i % 13 == 0) r.end = r.begin;            // a point
      if (i % 5 == 0) r.begin = 120.0f, r.end = 950.0f;  // many records in one cell
      if (i % 97 == 0) r.end = 3e7f;               // beyond the grid
      r.w_sh = std::pow(10.0, (int)(next() % 7) - 3) * (1 + next() % 1000) / 1000.0 * (next() % 4 != 0);
      r.w_ns = std::pow(10.0, (int)(next() % 7) - 3) * (1 + next() % 1000) / 1000.0;
      recs.push_back(r), block.push_back(k);
    }
  const long long n = (long long)recs.size();

  // the plain loop: per (kind, bb, be) and block a sum from 0.0 in record order
  std::map<std::tuple<int, int, int>, std::vector<double>> want;
  long long want_dropped = 0;
  for (long long i = 0; i < n; i++) {
    const int bb = bin_table(T, recs[i].begin), be = bin_table(T, recs[i].end);
    bad += bb != bin_libm(recs[i].begin) || std::min(be, COLATE_INTERVAL_BINS) != std::min(bin_libm(recs[i].end), COLATE_INTERVAL_BINS);
    if (be >= COLATE_INTERVAL_BINS) {
      want_dropped++;
      continue;
    }
    for (int kind = 0; kind < 2; kind++) {
      std::vector<double>& v = want[std::make_tuple(kind, bb, be)];
      v.resize(nb, 0.0);
      v[block[i]] += kind == 0 ? recs[i].w_sh : recs[i].w_ns;
    }
  }
  for (auto it = want.begin(); it != want.end();) {
    bool any = false;
    for (double x : it->second) any = any || x > 0.0;
    it = any ? std::next(it) : want.erase(it);
  }
  const int want_R = (int)want.size();
  double grid[COLATE_MAX_AGE_BINS];
  if (colate_age_grid(grid, COLATE_MAX_AGE_BINS) != COLATE_INTERVAL_BINS) return 1;

  // exactly enough room
  std::vector<int> kinds(want_R);
  std::vector<double> a0(want_R), a1(want_R), tab((size_t)nb * want_R);
  long long dropped = -1;
  const int R = colate_interval_cells_host(n, recs.data(), block.data(), nb, want_R, kinds.data(), a0.data(), a1.data(), tab.data(), &dropped);
  if (R != want_R || dropped != want_dropped) {
    std::fprintf(stderr, "R %d (want %d), dropped %lld (want %lld): %s\n", R, want_R, dropped, want_dropped, colate_last_error());
    return 1;
  }
  int r = 0;
  for (const auto& kv : want) {  // (the map's order is the rows': kind, bb, be)
    bad += kinds[r] != std::get<0>(kv.first) || a0[r] != grid[std::get<1>(kv.first)] || a1[r] != grid[std::get<2>(kv.first)];
    for (int k = 0; k < nb; k++) bad += std::memcmp(&tab[(size_t)k * R + r], &kv.second[k], sizeof(double)) != 0;
    r++;
  }
  std::printf("%lld records, %d rows, %lld dropped, %d mismatches\n", n, R, dropped, bad);

  // one row too few, no records, and refusals: nothing is written
  std::vector<int> k2(want_R, -7);
  std::vector<double> b0(want_R, -7.0), b1(want_R, -7.0), t2((size_t)nb * want_R, -7.0);
  long long d2 = -7;
  auto untouched = [&] {
    int u = d2 == -7;
    for (int x : k2) u = u && x == -7;
    for (double x : b0) u = u && x == -7.0;
    for (double x : b1) u = u && x == -7.0;
    for (double x : t2) u = u && x == -7.0;
    return u;
  };
  auto call = [&](int nb_, int room) {
    return colate_interval_cells_host(n, recs.data(), block.data(), nb_, room, k2.data(), b0.data(), b1.data(), t2.data(), &d2);
  };
  bad += call(nb, want_R - 1) != COLATE_EINVAL || !untouched();
  bad += call(0, want_R) != COLATE_EINVAL || !untouched();
  bad += call(2, want_R) != COLATE_EINVAL || !untouched();  // (block 2 outside [0, 2))
  const colate_interval_rec keep = recs[3];
  recs[3].begin = -1.0f;
  bad += call(nb, want_R) != COLATE_EINVAL || !untouched();
  recs[3] = keep, recs[3].end = NAN;
  bad += call(nb, want_R) != COLATE_EINVAL || !untouched();
  recs[3] = keep, recs[3].begin = 10.0f, recs[3].end = 5.0f;
  bad += call(nb, want_R) != COLATE_EINVAL || !untouched();
  recs[3] = keep, recs[3].w_sh = -1.0;
  bad += call(nb, want_R) != COLATE_EINVAL || !untouched();
  recs[3] = keep, recs[3].w_ns = INFINITY;
  bad += call(nb, want_R) != COLATE_EINVAL || !untouched();
  recs[3] = keep, block[3] = 1, block[4] = 0;
  bad += call(nb, want_R) != COLATE_EINVAL || !untouched();
  block[3] = block[4] = 0;
  bad += colate_interval_cells_host(0, nullptr, nullptr, 1, 0, nullptr, nullptr, nullptr, nullptr, &d2) != 0 || d2 != 0;
  if (bad) {
    std::fprintf(stderr, "%d mismatches\n", bad);
    return 1;
  }
  std::printf("ok\n");
  return 0;
}
