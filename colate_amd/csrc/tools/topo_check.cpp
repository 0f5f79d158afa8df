// colate_amd/csrc/tools/topo_check.cpp -- stand-alone run of the two host forms of `Colate --mode count_topo` (count_topo.h)
// against each other:
//   * small synthetic inputs, its own variant of tools/topo_inputs.hpp (three chromosomes, four .colate.in files; rows at equal positions, rows with equal
//     ages and with a negative age_end, which this mode searches, flipped, two-branch and descending-age rows, which it does not;
//     two samples end before their chromosomes' last rows, so their conditioning record is the next chromosome's first or the
//     file's last), read, decoded and indexed by the loader of the command line (load_walk_inputs with RowSet::count_topo);
//   * the cursor walk (topo_cursor_triples) against topo_view_host on the loader's view and against colate_topo_samples_host
//     on back-to-back copies: every line of every triple -- row, sign, the conditioning record's counts -- and every triple's
//     qualifying rows, with a stream exactly as long as the longest triple needs;
//   * the refusals of the call by name, nothing written; the device form ends in COLATE_ENODEVICE in this build.
// For the host sanitizer build (`make asan`: bin/topo_check_asan, linked with tools/no_device_stubs.cpp); prints "ok" and exits 0
// when everything agrees.  Usage: topo_check_asan DIR (an existing, writable directory).
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "colate_amd.h"
#include "count_topo.h"
#include "cli_lists.h"
#include "topo_inputs.hpp"
#include "walk_inputs.h"

namespace {

using topo_inputs::TopoInputs;
using topo_inputs::triples_of;
using topo_inputs::write_inputs;

bool same_line(const colate_drv::TopoLine& a, const colate_drv::TopoLine& b) {
  return a.chr == b.chr && a.pos == b.pos && a.age_begin == b.age_begin && a.age_end == b.age_end && a.sign == b.sign && a.DAF == b.DAF && a.N == b.N;
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
  const std::vector<std::string> names = {"1", "2", "3"};
  if (!write_inputs(dir, names, 300, TopoInputs{9753, true})) {
    std::fprintf(stderr, "cannot write the inputs under %s\n", dir.c_str());
    return 1;
  }
  std::vector<std::string> mut_files;
  for (const std::string& c : names) mut_files.push_back(dir + "/P_chr" + c + ".mut");
  const std::vector<PairSpec> triples = triples_of(dir);
  const int P = (int)triples.size(), C = (int)names.size();
  const unsigned seed = 77;

  WalkInputs in;
  if (!load_walk_inputs(names, mut_files, triples, in, RowSet::count_topo) || !in.indexed || !in.files_ok || in.S != 4 || (int)in.cond_ids.size() != P ||
      in.cidx_ptrs.size() != (size_t)in.S * C) {
    std::fprintf(stderr, "the inputs were not indexed (%d samples)\n", in.S);
    return 1;
  }
  std::vector<std::vector<TopoLine>> want;
  std::vector<long long> want_draws;
  if (!topo_cursor_triples(in, names, triples, seed, want, want_draws)) return 1;
  long long most = 0, lines = 0, unmatched = 0;
  for (int p = 0; p < P; p++) most = std::max(most, want_draws[(size_t)p]), lines += (long long)want[(size_t)p].size();
  if (most < 50 || lines < 100) {
    std::fprintf(stderr, "%lld qualifying rows at most, %lld lines\n", most, lines);
    return 1;
  }
  std::vector<double> u((size_t)(2 * most));  // exactly as long as the longest triple needs
  {
    std::mt19937 rng(seed);
    std::uniform_real_distribution<double> dist_unif(0, 1);
    for (double& x : u) x = dist_unif(rng);
  }
  std::vector<colate_topo::Triple> ids((size_t)P);
  for (int p = 0; p < P; p++) ids[(size_t)p] = colate_topo::Triple{in.cond_ids[(size_t)p], in.pairs[(size_t)p].target, in.pairs[(size_t)p].reference};
  std::vector<long long> word_off((size_t)C + 1);
  const long long words = colate_iw::mask_words(C, in.row_off.data(), word_off.data());
  const long long cap = P * words;

  // planes into lines, as the command line does it
  auto compare = [&](const char* what, const std::vector<long long>& wo, const std::vector<unsigned long long>& plus,
                     const std::vector<unsigned long long>& minus, const std::vector<long long>& draws) {
    if (wo != word_off || draws != want_draws) {
      std::fprintf(stderr, "%s: word offsets or qualifying rows differ\n", what);
      bad++;
      return;
    }
    for (int p = 0; p < P; p++) {
      std::vector<TopoLine> got;
      for (int c = 0; c < C; c++) {
        const colate_walk_idx* const ci = in.cidx_ptrs[(size_t)ids[(size_t)p].cond * C + c];
        const colate_walk_idx* const xi = in.idx_ptrs[(size_t)ids[(size_t)p].cond * C + c];
        for (long long k = word_off[(size_t)c]; k < word_off[(size_t)c + 1]; k++) {
          const unsigned long long a = plus[(size_t)(p * words + k)], b = minus[(size_t)(p * words + k)];
          bad += (a & b) != 0;
          for (unsigned long long q = a | b; q; q &= q - 1) {
            const int bit = __builtin_ctzll(q);
            const long long i = (k - word_off[(size_t)c]) * 64 + bit;
            const colate_walk_row& r = in.row_ptrs[(size_t)c][i];
            got.push_back(TopoLine{c, r.pos, r.age_begin, r.age_end, (a >> bit) & 1 ? 1 : -1, (int)ci[i].DAF, (int)ci[i].DAF + (int)ci[i].AAF});
            unmatched += (xi[i].DAF | xi[i].AAF) == 0;  // the conditioning record is not the row's
          }
        }
      }
      bool same = got.size() == want[(size_t)p].size();
      for (size_t k = 0; same && k < got.size(); k++) same = same_line(got[k], want[(size_t)p][k]);
      if (!same) {
        std::fprintf(stderr, "%s: triple %d: %zu lines (the cursor walk: %zu), or a line differs\n", what, p, got.size(), want[(size_t)p].size());
        bad++;
      }
    }
  };
  colate_topo::View v;
  v.C = C, v.row_off = in.row_off.data(), v.rows = in.row_ptrs.data(), v.S = in.S, v.idx = in.idx_ptrs.data(), v.cidx = in.cidx_ptrs.data();
  v.P = P, v.triples = ids.data(), v.n_uniforms = (long long)u.size(), v.uniforms = u.data();
  {
    std::vector<long long> wo((size_t)C + 1, -1), draws((size_t)P, -1);
    std::vector<unsigned long long> plus((size_t)cap, ~0ull), minus((size_t)cap, ~0ull);
    if (int rc = colate_topo::topo_view_host(v, cap, wo.data(), plus.data(), minus.data(), draws.data())) {
      std::fprintf(stderr, "topo_view_host: %d (%s)\n", rc, colate_last_error());
      return 1;
    }
    compare("view", wo, plus, minus, draws);
  }
  bad += unmatched < 1;

  // ---- the C entry point on back-to-back copies
  const long long nrows = in.row_off.back();
  std::vector<colate_walk_idx> idx((size_t)in.S * nrows), cidx((size_t)in.S * nrows);
  for (int c = 0; c < C; c++) {
    const size_t nc = (size_t)(in.row_off[(size_t)c + 1] - in.row_off[(size_t)c]);
    for (int s = 0; s < in.S; s++) {
      std::memcpy(&idx[(size_t)s * nrows + in.row_off[(size_t)c]], in.idx_ptrs[(size_t)s * C + c], nc * sizeof(colate_walk_idx));
      std::memcpy(&cidx[(size_t)s * nrows + in.row_off[(size_t)c]], in.cidx_ptrs[(size_t)s * C + c], nc * sizeof(colate_walk_idx));
    }
  }
  auto flat = [&](const long long* row_off, const colate_walk_row* rows, const colate_walk_idx* ci, const colate_topo_triple* tr, long long nu,
                  const double* uu, long long room, std::vector<long long>& wo, std::vector<unsigned long long>& plus,
                  std::vector<unsigned long long>& minus, std::vector<long long>& draws, bool device = false) {
    return (device ? colate_topo_samples : colate_topo_samples_host)(C, row_off, rows, in.S, idx.data(), ci, P, tr, nu, uu, room, wo.data(), plus.data(),
                                                                    minus.data(), draws.data());
  };
  {
    std::vector<long long> wo((size_t)C + 1, -1), draws((size_t)P, -1);
    std::vector<unsigned long long> plus((size_t)cap, ~0ull), minus((size_t)cap, ~0ull);
    if (int rc = flat(in.row_off.data(), in.rows.data(), cidx.data(), ids.data(), (long long)u.size(), u.data(), cap, wo, plus, minus, draws)) {
      std::fprintf(stderr, "colate_topo_samples_host: %d (%s)\n", rc, colate_last_error());
      return 1;
    }
    compare("C entry point", wo, plus, minus, draws);
  }

  // ---- refusals: the code, the name, nothing written
  auto refused = [&](const char* what, int code, const long long* row_off, const colate_walk_row* rows, const colate_walk_idx* ci,
                     const colate_topo_triple* tr, long long nu, const double* uu, long long room, bool device = false) {
    std::vector<long long> wo((size_t)C + 1, -7), draws((size_t)P, -7);
    std::vector<unsigned long long> plus((size_t)cap, 7), minus((size_t)cap, 7);
    const int rc = flat(row_off, rows, ci, tr, nu, uu, room, wo, plus, minus, draws, device);
    bool untouched = true;
    for (long long x : wo) untouched = untouched && x == -7;
    for (long long x : draws) untouched = untouched && x == -7;
    for (unsigned long long x : plus) untouched = untouched && x == 7;
    for (unsigned long long x : minus) untouched = untouched && x == 7;
    if (rc != code || !std::strstr(colate_last_error(), what) || !untouched) {
      std::fprintf(stderr, "refusal `%s`: rc %d, message `%s`, outputs %s\n", what, rc, colate_last_error(), untouched ? "untouched" : "written");
      bad++;
    }
  };
  const long long nu = (long long)u.size();
  std::vector<colate_topo_triple> tr = ids;
  tr[2].cond = in.S;
  refused("triple 2: sample id out of range", COLATE_EINVAL, in.row_off.data(), in.rows.data(), cidx.data(), tr.data(), nu, u.data(), cap);
  tr = ids, tr[4].reference = -1;
  refused("triple 4: sample id out of range", COLATE_EINVAL, in.row_off.data(), in.rows.data(), cidx.data(), tr.data(), nu, u.data(), cap);
  std::vector<long long> ro2 = in.row_off;
  ro2[1] = ro2[2] + 1;
  refused("row_off decreases at chromosome 1", COLATE_EINVAL, ro2.data(), in.rows.data(), cidx.data(), ids.data(), nu, u.data(), cap);
  refused("NULL pointer", COLATE_EINVAL, in.row_off.data(), nullptr, cidx.data(), ids.data(), nu, u.data(), cap);
  refused("NULL pointer", COLATE_EINVAL, in.row_off.data(), in.rows.data(), nullptr, ids.data(), nu, u.data(), cap);
  refused("NULL pointer", COLATE_EINVAL, in.row_off.data(), in.rows.data(), cidx.data(), nullptr, nu, u.data(), cap);
  refused("NULL pointer", COLATE_EINVAL, in.row_off.data(), in.rows.data(), cidx.data(), ids.data(), nu, nullptr, cap);
  refused("n_uniforms = -1", COLATE_EINVAL, in.row_off.data(), in.rows.data(), cidx.data(), ids.data(), -1, u.data(), cap);
  refused("needed: ", COLATE_ELIMIT, in.row_off.data(), in.rows.data(), cidx.data(), ids.data(), nu, u.data(), cap - 1);
  char needed[64];
  std::snprintf(needed, sizeof(needed), "(needed: %lld)", nu);
  refused(needed, COLATE_ELIMIT, in.row_off.data(), in.rows.data(), cidx.data(), ids.data(), nu - 1, u.data(), cap);  // one uniform short
  refused("no device", COLATE_ENODEVICE, in.row_off.data(), in.rows.data(), cidx.data(), ids.data(), nu, u.data(), cap, true);

  std::printf("%d triples over %d samples, %lld rows, %lld lines, %lld qualifying rows at most, %lld printed rows off the conditioning record\n", P,
              in.S, nrows, lines, most, unmatched);
  if (bad) {
    std::fprintf(stderr, "%d mismatches\n", bad);
    return 1;
  }
  std::printf("ok\n");
  return 0;
}
