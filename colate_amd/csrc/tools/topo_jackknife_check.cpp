// colate_amd/csrc/tools/topo_jackknife_check.cpp -- stand-alone run of the host forms of `Colate --mode count_topo --jackknife`
// (count_topo.h: the blocks of this mode, colate_topo_profile_blocks, colate_topo_jackknife) against each other:
//   * small synthetic inputs, its own variant of tools/topo_inputs.hpp (three chromosomes, four .colate.in files; rows at equal positions, rows with equal ages
//     and with negative ages; two samples end before their chromosomes' last rows), read, decoded and indexed by the loader of the
//     command line (load_walk_inputs with RowSet::count_topo);
//   * the blocks: topo_cursor_blocks on the loaded rows against colate_topo_blocks on the indexed ones, for several block sizes;
//   * the cursor walk (topo_cursor_triples) binned by block in its `drew` and `emit` sinks against topo_profile_blocks_host on the
//     loader's view and colate_topo_profile_blocks_host on back-to-back copies, and the sums over the blocks against the cursor
//     walk's own profile, for the epochs of `--age_profile 1,4,0.5`, for one epoch and for 1024, with a stream exactly as long as
//     the longest triple needs;
//   * the jackknife of every triple: finite D where a line was printed, the NaN rules, plus and minus swapped;
//   * the refusals of the calls by name, nothing written; the device form ends in COLATE_ENODEVICE in this build.
// For the host sanitizer build (bin/topo_jackknife_check_asan, linked with tools/no_device_stubs.cpp); prints "ok" and exits 0 when
// everything agrees.  Usage: topo_jackknife_check_asan DIR (an existing, writable directory).
#include <algorithm>
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

bool same(double x, double y) { return (std::isnan(x) && std::isnan(y)) || std::memcmp(&x, &y, sizeof(x)) == 0; }

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
  if (!write_inputs(dir, names, 300, TopoInputs{97531, false, true})) {
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
  std::vector<std::vector<double>> epoch_sets(3);
  epoch_sets[0].resize(COLATE_MAX_EPOCHS);
  const int E0 = colate_epochs_from_bins("1,4,0.5", 0.0, 28.0, epoch_sets[0].data(), COLATE_MAX_EPOCHS, nullptr);
  if (E0 < 3) {
    std::fprintf(stderr, "colate_epochs_from_bins: %d (%s)\n", E0, colate_last_error());
    return 1;
  }
  epoch_sets[0].resize((size_t)E0);
  epoch_sets[0][0] = -1.0;  // (as the command line calls: age_epoch reads none but epochs[1 .. E - 1])
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
  // ---- the blocks: the cursor path's against the call's, a block per base of the gap among them
  const int sizes[] = {30000000, 100000, 7001, 13};
  long long empty_blocks = 0;
  for (int nbpb : sizes) {
    std::vector<int> a, b((size_t)C + 1, -1);
    const int ra = topo_cursor_blocks(in, nbpb, a), rb = colate_topo_blocks(C, in.row_off.data(), in.rows.data(), nbpb, b.data());
    if (nbpb == 13) {  // more than 65535 blocks: both refuse by name
      bad += ra != COLATE_ELIMIT || rb != COLATE_ELIMIT || !std::strstr(colate_last_error(), "(needed: ") || b[0] != -1;
      continue;
    }
    if (ra || rb || a != b) {
      std::fprintf(stderr, "blocks of %d bases: %d, %d (%s)\n", nbpb, ra, rb, colate_last_error());
      bad++;
    }
  }

  std::vector<double> u;
  std::vector<long long> want_draws;
  long long most = 0, lines_in_all = 0, defined = 0;
  for (const std::vector<double>& ep : epoch_sets)
    for (int nbpb : {30000000, 100000, 7001}) {
      const int E = (int)ep.size();
      if (E == colate_topo::kMaxProfileEpochs && nbpb == 7001) continue;  // (300 blocks x 1024 epochs x 7 triples say nothing the others do not)
      std::vector<int> blk_off;
      if (int rc = topo_cursor_blocks(in, nbpb, blk_off)) return std::fprintf(stderr, "blocks: %d\n", rc), 1;
      const int nb = blk_off[(size_t)C];
      const size_t per_block = (size_t)E * 3;
      TopoProfile want;
      want.E = E, want.epochs = ep.data(), want.nbpb = nbpb, want.blk_off = blk_off.data();
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
      bad += want.blocks.size() != (size_t)P * nb * per_block;
      // the sums over the blocks are the walk's own profile; the lines binned here by their position are its plus and minus
      for (int p = 0; p < P; p++) {
        std::vector<long long> sum(per_block, 0), binned((size_t)nb * E * 2, 0);
        for (int b = 0; b < nb; b++)
          for (size_t k = 0; k < per_block; k++) sum[k] += want.blocks[((size_t)p * nb + b) * per_block + k];
        for (size_t k = 0; k < per_block; k++) bad += sum[k] != want.counts[(size_t)p * per_block + k];
        for (const TopoLine& l : lines[(size_t)p])
          binned[((size_t)(blk_off[(size_t)l.chr] + colate_iw::block_of_pos(l.pos, nbpb)) * E + colate_topo::age_epoch(l.age_begin, l.age_end, ep.data(), E)) * 2 +
                 (l.sign > 0 ? 0 : 1)]++;
        for (size_t k = 0; k < (size_t)nb * E; k++) {
          const long long* const x = &want.blocks[((size_t)p * nb * E + k) * 3];
          bad += x[0] != binned[k * 2] || x[1] != binned[k * 2 + 1] || x[0] + x[1] > x[2];
        }
      }
      if (nbpb == 100000 && E == E0)
        for (int b = 0; b < nb; b++) {
          long long rows_in = 0;
          for (int p = 0; p < P; p++)
            for (int e = 0; e < E; e++) rows_in += want.blocks[(((size_t)p * nb + b) * E + e) * 3 + 2];
          empty_blocks += rows_in == 0;
        }
      colate_topo::View v;
      v.C = C, v.row_off = in.row_off.data(), v.rows = in.row_ptrs.data(), v.S = in.S, v.idx = in.idx_ptrs.data(), v.cidx = in.cidx_ptrs.data();
      v.P = P, v.triples = ids.data(), v.n_uniforms = (long long)u.size(), v.uniforms = u.data();
      for (int form = 0; form < 2; form++) {
        std::vector<long long> counts((size_t)P * nb * per_block, -1), draws((size_t)P, -1);
        const int rc = form == 0 ? colate_topo::topo_profile_blocks_host(v, E, ep.data(), nbpb, nb, counts.data(), draws.data())
                                 : colate_topo_profile_blocks_host(C, in.row_off.data(), in.rows.data(), in.S, idx.data(), cidx.data(), P, ids.data(),
                                                                   (long long)u.size(), u.data(), E, ep.data(), nbpb, nb, counts.data(), draws.data());
        if (rc) {
          std::fprintf(stderr, "profile blocks host form %d: %d (%s)\n", form, rc, colate_last_error());
          return 1;
        }
        if (counts != want.blocks || draws != want_draws) {
          std::fprintf(stderr, "E = %d, %d bases per block, form %d: the counts or the qualifying rows differ from the cursor walk's\n", E, nbpb, form);
          bad++;
        }
      }
      // ---- the jackknife of every triple, through the C entry point and the internal one; plus and minus swapped
      for (int p = 0; p < P; p++) {
        const long long* const mine = &want.blocks[(size_t)p * nb * per_block];
        std::vector<double> out(((size_t)E + 1) * 4, -5.0), out2 = out, swapped_out = out;
        std::vector<int> used((size_t)E + 1, -5), used2 = used;
        if (int rc = colate_topo_jackknife(nb, E, mine, out.data(), used.data())) return std::fprintf(stderr, "jackknife: %d\n", rc), 1;
        colate_topo::jackknife(nb, E, mine, out2.data(), used2.data());
        std::vector<long long> swapped(mine, mine + (size_t)nb * per_block);
        for (size_t k = 0; k < (size_t)nb * E; k++) std::swap(swapped[k * 3], swapped[k * 3 + 1]);
        colate_topo::jackknife(nb, E, swapped.data(), swapped_out.data(), used2.data());
        for (int cell = 0; cell <= E; cell++) {
          const double* const o = &out[(size_t)cell * 4];
          long long n = 0;
          int g = 0;
          for (int b = 0; b < nb; b++) {
            long long nj = 0;
            for (int e = cell < E ? cell : 0; e < (cell < E ? cell + 1 : E); e++) nj += mine[((size_t)b * E + e) * 3] + mine[((size_t)b * E + e) * 3 + 1];
            n += nj, g += nj > 0;
          }
          bad += used[(size_t)cell] != g || used2[(size_t)cell] != g;
          bad += std::isnan(o[0]) != (n == 0) || (g < 2 && !(std::isnan(o[1]) && std::isnan(o[2]) && std::isnan(o[3])));
          bad += g >= 2 && (!std::isfinite(o[1]) || !(o[2] >= 0) || std::isnan(o[3]) != !(o[2] > 0));
          for (int k = 0; k < 4; k++) {
            bad += !same(o[k], out2[(size_t)cell * 4 + k]);
            const double sw = swapped_out[(size_t)cell * 4 + k], neg = k == 2 ? o[k] : -o[k];  // (a zero keeps its sign: 0 / n is +0 both ways)
            bad += !(same(sw, neg) || (sw == 0.0 && neg == 0.0));
          }
          defined += g >= 2;
        }
      }
    }
  bad += empty_blocks < 2 || defined < 20;  // (the gap left blocks without a row; the statistic was defined somewhere)

  // ---- refusals: the code, the name, nothing written
  const std::vector<double>& ep = epoch_sets[0];
  std::vector<int> blk_off;
  if (topo_cursor_blocks(in, 100000, blk_off)) return 1;
  const int nb = blk_off[(size_t)C];
  auto refused = [&](const char* what, int code, int E, const double* epochs, long long nu, int nbpb, int nb_given, bool with_counts, bool with_draws,
                     bool device = false) {
    std::vector<long long> counts((size_t)P * ((size_t)nb + 1) * 64 * 3, -7), draws((size_t)P, -7);
    const int rc = (device ? colate_topo_profile_blocks : colate_topo_profile_blocks_host)(
        C, in.row_off.data(), in.rows.data(), in.S, idx.data(), cidx.data(), P, ids.data(), nu, u.data(), E, epochs, nbpb, nb_given,
        with_counts ? counts.data() : nullptr, with_draws ? draws.data() : nullptr);
    bool untouched = true;
    for (long long x : counts) untouched = untouched && x == -7;
    for (long long x : draws) untouched = untouched && x == -7;
    if (rc != code || !std::strstr(colate_last_error(), what) || !untouched) {
      std::fprintf(stderr, "refusal `%s`: rc %d, message `%s`, outputs %s\n", what, rc, colate_last_error(), untouched ? "untouched" : "written");
      bad++;
    }
  };
  const long long nu = (long long)u.size();
  refused("E = 0 epochs", COLATE_EINVAL, 0, ep.data(), nu, 100000, nb, true, true);
  std::vector<double> e2 = ep;
  e2[3] = e2[2];
  refused("epochs[3]", COLATE_EINVAL, E0, e2.data(), nu, 100000, nb, true, true);
  refused("NULL pointer", COLATE_EINVAL, E0, nullptr, nu, 100000, nb, true, true);
  refused("NULL pointer", COLATE_EINVAL, E0, ep.data(), nu, 100000, nb, false, true);
  refused("NULL pointer", COLATE_EINVAL, E0, ep.data(), nu, 100000, nb, true, false);
  refused("num_bases_per_block = 0", COLATE_EINVAL, E0, ep.data(), nu, 0, nb, true, true);
  refused("num_bases_per_block = -3", COLATE_EINVAL, E0, ep.data(), nu, -3, nb, true, true);
  refused("at or above 2^31 - num_bases_per_block", COLATE_EINVAL, E0, ep.data(), nu, 2147483647, 3, true, true);
  refused("(needed: ", COLATE_ELIMIT, E0, ep.data(), nu, 13, nb, true, true);
  refused("is not the", COLATE_EINVAL, E0, ep.data(), nu, 100000, nb + 1, true, true);
  refused("is not the", COLATE_EINVAL, E0, ep.data(), nu, 100000, nb - 1, true, true);
  char needed[64];
  std::snprintf(needed, sizeof(needed), "(needed: %lld)", nu);
  refused(needed, COLATE_ELIMIT, E0, ep.data(), nu - 1, 100000, nb, true, true);  // one uniform short
  refused("no device", COLATE_ENODEVICE, E0, ep.data(), nu, 100000, nb, true, true, true);
  {
    double out[8];
    int used[2];
    const long long one[3] = {1, 2, 3}, neg[3] = {1, -2, 3};
    bad += colate_topo_jackknife(0, 1, one, out, used) != COLATE_EINVAL || colate_topo_jackknife(1, 0, one, out, used) != COLATE_EINVAL;
    bad += colate_topo_jackknife(1, 1, nullptr, out, used) != COLATE_EINVAL || colate_topo_jackknife(1, 1, one, nullptr, used) != COLATE_EINVAL;
    bad += colate_topo_jackknife(1, 1, neg, out, used) != COLATE_EINVAL || !std::strstr(colate_last_error(), "is negative");
    bad += colate_topo_jackknife(1, 1, one, out, used) != COLATE_OK || used[0] != 1 || used[1] != 1 || !(out[0] < 0) || !std::isnan(out[1]);
  }

  std::printf("%d triples over %d samples, %lld rows, %lld lines, %lld qualifying rows at most, %d blocks of 100000 bases of which %lld hold no row, %lld cells with a "
              "jackknife\n", P, in.S, nrows, lines_in_all, most, nb, empty_blocks, defined);
  if (bad) {
    std::fprintf(stderr, "%d mismatches\n", bad);
    return 1;
  }
  std::printf("ok\n");
  return 0;
}
