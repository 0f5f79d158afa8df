// colate_amd/csrc/tools/topo_profile_check.cpp -- stand-alone run of the host forms of the age profile of `Colate --mode count_topo`
// (count_topo.h: age_epoch, colate_topo_profile) against each other:
//   * small synthetic inputs, its own variant of tools/topo_inputs.hpp (three chromosomes, four .colate.in files; rows at equal positions, rows with equal
//     ages and with negative ages, which this mode searches; two samples end before their chromosomes' last rows), read, decoded
//     and indexed by the loader of the command line (load_walk_inputs with RowSet::count_topo);
//   * the cursor walk (topo_cursor_triples): its lines binned here by age_epoch, and the counts it forms itself -- plus, minus and
//     qualifying rows per (triple, epoch) -- against topo_profile_host on the loader's view and colate_topo_profile_host on
//     back-to-back copies, for the epochs of `--age_profile 1,4,0.5`, for one epoch and for 1024, with a stream exactly as long
//     as the longest triple needs;
//   * the refusals of the call by name, nothing written; the device form ends in COLATE_ENODEVICE in this build.
// For the host sanitizer build (bin/topo_profile_check_asan, linked with tools/no_device_stubs.cpp); prints "ok" and exits 0 when
// everything agrees.  Usage: topo_profile_check_asan DIR (an existing, writable directory).
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
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
  if (!write_inputs(dir, names, 300, TopoInputs{24681})) {
    std::fprintf(stderr, "cannot write the inputs under %s\n", dir.c_str());
    return 1;
  }
  std::vector<std::string> mut_files;
  for (const std::string& c : names) mut_files.push_back(dir + "/P_chr" + c + ".mut");
  const std::vector<PairSpec> triples = triples_of(dir);
  const int P = (int)triples.size(), C = (int)names.size();
  const unsigned seed = 78;

  WalkInputs in;
  if (!load_walk_inputs(names, mut_files, triples, in, RowSet::count_topo) || !in.indexed || !in.files_ok || in.S != 4 || (int)in.cond_ids.size() != P ||
      in.cidx_ptrs.size() != (size_t)in.S * C) {
    std::fprintf(stderr, "the inputs were not indexed (%d samples)\n", in.S);
    return 1;
  }
  // the three sets of epochs: those of the command line, one epoch, and the most a call takes
  std::vector<std::vector<double>> epoch_sets(3);
  epoch_sets[0].resize(COLATE_MAX_EPOCHS);
  const int E0 = colate_epochs_from_bins("1,4,0.5", 0.0, 28.0, epoch_sets[0].data(), COLATE_MAX_EPOCHS, nullptr);
  if (E0 < 3) {
    std::fprintf(stderr, "colate_epochs_from_bins: %d (%s)\n", E0, colate_last_error());
    return 1;
  }
  epoch_sets[0].resize((size_t)E0);
  epoch_sets[0][0] = -1.0;  // (the reference's epochs start 0, 0; age_epoch reads none but epochs[1 .. E - 1]: as the command line calls)
  epoch_sets[1] = {0.0};
  for (int e = 0; e < colate_topo::kMaxProfileEpochs; e++) epoch_sets[2].push_back(e * 7.5);

  std::vector<colate_topo::Triple> ids((size_t)P);
  for (int p = 0; p < P; p++) ids[(size_t)p] = colate_topo::Triple{in.cond_ids[(size_t)p], in.pairs[(size_t)p].target, in.pairs[(size_t)p].reference};
  const long long nrows = in.row_off.back();
  std::vector<colate_walk_idx> idx((size_t)in.S * nrows), cidx((size_t)in.S * nrows);
  for (int c = 0; c < C; c++) {
    const size_t nc = (size_t)(in.row_off[(size_t)c + 1] - in.row_off[(size_t)c]);
    for (int s = 0; s < in.S; s++) {
      std::memcpy(&idx[(size_t)s * nrows + in.row_off[(size_t)c]], in.idx_ptrs[(size_t)s * C + c], nc * sizeof(colate_walk_idx));
      std::memcpy(&cidx[(size_t)s * nrows + in.row_off[(size_t)c]], in.cidx_ptrs[(size_t)s * C + c], nc * sizeof(colate_walk_idx));
    }
  }
  std::vector<double> u;
  std::vector<long long> want_draws;
  long long most = 0, lines_in_all = 0, bins_used = 0;
  for (const std::vector<double>& ep : epoch_sets) {
    const int E = (int)ep.size();
    TopoProfile want;
    want.E = E, want.epochs = ep.data();
    std::vector<std::vector<TopoLine>> lines;
    if (!topo_cursor_triples(in, names, triples, seed, lines, want_draws, &want)) return 1;
    if (u.empty()) {
      for (int p = 0; p < P; p++) most = std::max(most, want_draws[(size_t)p]), lines_in_all += (long long)lines[(size_t)p].size();
      if (most < 50 || lines_in_all < 100) {
        std::fprintf(stderr, "%lld qualifying rows at most, %lld lines\n", most, lines_in_all);
        return 1;
      }
      u.resize((size_t)(2 * most));  // exactly as long as the longest triple needs
      std::mt19937 rng(seed);
      std::uniform_real_distribution<double> dist_unif(0, 1);
      for (double& x : u) x = dist_unif(rng);
    }
    // the cursor walk's lines, binned here: the plus and minus columns of its own counts
    for (int p = 0; p < P; p++) {
      std::vector<long long> binned((size_t)E * 2, 0);
      for (const TopoLine& l : lines[(size_t)p]) binned[(size_t)colate_topo::age_epoch(l.age_begin, l.age_end, ep.data(), E) * 2 + (l.sign > 0 ? 0 : 1)]++;
      long long qualifying = 0;
      for (int e = 0; e < E; e++) {
        const long long* const x = &want.counts[((size_t)p * E + e) * 3];
        bad += x[0] != binned[(size_t)e * 2] || x[1] != binned[(size_t)e * 2 + 1] || x[0] + x[1] > x[2];
        qualifying += x[2];
        if (E == E0 && p == 0) bins_used += x[2] > 0;
      }
      bad += qualifying != want_draws[(size_t)p];
    }
    colate_topo::View v;
    v.C = C, v.row_off = in.row_off.data(), v.rows = in.row_ptrs.data(), v.S = in.S, v.idx = in.idx_ptrs.data(), v.cidx = in.cidx_ptrs.data();
    v.P = P, v.triples = ids.data(), v.n_uniforms = (long long)u.size(), v.uniforms = u.data();
    for (int form = 0; form < 2; form++) {
      std::vector<long long> counts((size_t)P * E * 3, -1), draws((size_t)P, -1);
      const int rc = form == 0 ? colate_topo::topo_profile_host(v, E, ep.data(), counts.data(), draws.data())
                               : colate_topo_profile_host(C, in.row_off.data(), in.rows.data(), in.S, idx.data(), cidx.data(), P, ids.data(),
                                                          (long long)u.size(), u.data(), E, ep.data(), counts.data(), draws.data());
      if (rc) {
        std::fprintf(stderr, "profile host form %d: %d (%s)\n", form, rc, colate_last_error());
        return 1;
      }
      if (counts != want.counts || draws != want_draws) {
        std::fprintf(stderr, "E = %d, form %d: the counts or the qualifying rows differ from the cursor walk's\n", E, form);
        bad++;
      }
    }
  }
  bad += bins_used < 4;  // (the rows spread over the epochs of the command line)

  // ---- refusals: the code, the name, nothing written
  const std::vector<double>& ep = epoch_sets[0];
  auto refused = [&](const char* what, int code, int E, const double* epochs, long long nu, bool with_counts, bool with_draws, bool device = false) {
    std::vector<long long> counts((size_t)P * colate_topo::kMaxProfileEpochs * 3, -7), draws((size_t)P, -7);
    const int rc = (device ? colate_topo_profile : colate_topo_profile_host)(C, in.row_off.data(), in.rows.data(), in.S, idx.data(), cidx.data(), P, ids.data(),
                                                                            nu, u.data(), E, epochs, with_counts ? counts.data() : nullptr,
                                                                            with_draws ? draws.data() : nullptr);
    bool untouched = true;
    for (long long x : counts) untouched = untouched && x == -7;
    for (long long x : draws) untouched = untouched && x == -7;
    if (rc != code || !std::strstr(colate_last_error(), what) || !untouched) {
      std::fprintf(stderr, "refusal `%s`: rc %d, message `%s`, outputs %s\n", what, rc, colate_last_error(), untouched ? "untouched" : "written");
      bad++;
    }
  };
  const long long nu = (long long)u.size();
  refused("E = 0 epochs", COLATE_EINVAL, 0, ep.data(), nu, true, true);
  refused("E = 1025 epochs", COLATE_EINVAL, 1025, epoch_sets[2].data(), nu, true, true);
  std::vector<double> e2 = ep;
  e2[3] = e2[2];
  refused("epochs[3]", COLATE_EINVAL, E0, e2.data(), nu, true, true);
  e2 = ep, std::swap(e2[1], e2[2]);
  refused("epochs[2]", COLATE_EINVAL, E0, e2.data(), nu, true, true);
  e2 = ep, e2[(size_t)E0 - 1] = std::numeric_limits<double>::infinity();
  refused("is not finite", COLATE_EINVAL, E0, e2.data(), nu, true, true);
  e2 = ep, e2[1] = std::nan("");
  refused("epochs[1] is not finite", COLATE_EINVAL, E0, e2.data(), nu, true, true);
  refused("NULL pointer", COLATE_EINVAL, E0, nullptr, nu, true, true);
  refused("NULL pointer", COLATE_EINVAL, E0, ep.data(), nu, false, true);
  refused("NULL pointer", COLATE_EINVAL, E0, ep.data(), nu, true, false);
  char needed[64];
  std::snprintf(needed, sizeof(needed), "(needed: %lld)", nu);
  refused(needed, COLATE_ELIMIT, E0, ep.data(), nu - 1, true, true);  // one uniform short
  refused("no device", COLATE_ENODEVICE, E0, ep.data(), nu, true, true, true);

  std::printf("%d triples over %d samples, %lld rows, %lld lines, %lld qualifying rows at most, %d epochs of which triple 0 fills %lld\n", P, in.S, nrows,
              lines_in_all, most, E0, bins_used);
  if (bad) {
    std::fprintf(stderr, "%d mismatches\n", bad);
    return 1;
  }
  std::printf("ok\n");
  return 0;
}
