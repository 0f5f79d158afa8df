// colate_amd/csrc/tools/topo_expected_check.cpp -- stand-alone run of the host forms of `Colate --mode count_topo --expected`
// (count_topo.h: the expected counts, colate_topo_expected_blocks) against each other:
//   * small synthetic inputs, its own variant of tools/topo_inputs.hpp (three chromosomes, four .colate.in files; rows at equal positions, rows with equal ages
//     and with negative ages; a gap that leaves blocks without a row; two samples end before their chromosomes' last rows), read,
//     decoded and indexed by the loader of the command line (load_walk_inputs with RowSet::count_topo);
//   * the cursor path (topo_cursor_expected: the walk's `drew` sink forms the addends from the cursors' counts) against
//     topo_expected_blocks_host on the loader's view and colate_topo_expected_blocks_host on back-to-back copies, for every triple,
//     for the epochs of `--age_profile 1,4,0.5`, for one epoch and for 1024, at three block sizes; the sums over the blocks against
//     the walk's own; the qualifying rows against those of the sampled cursor walk (topo_cursor_triples);
//   * the same inputs with every count multiplied by 70000 -- beyond the 16 bits of a walk index, so no file is indexed and the
//     addends take the 128-bit intermediate --: the quotients are those of the small counts, and so is every integer;
//   * expected_addends against a 128-bit quotient on counts at the edges of 16 and of 32 bits;
//   * the refusals of the call by name, nothing written; the device form ends in COLATE_ENODEVICE in this build.
// For the host sanitizer build (bin/topo_expected_check_asan, linked with tools/no_device_stubs.cpp); prints "ok" and exits 0 when
// everything agrees.  Usage: topo_expected_check_asan DIR (an existing, writable directory).
#include <sys/stat.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
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

using colate_drv::PairSpec;

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) {
    std::fprintf(stderr, "usage: %s DIR\n", argv[0]);
    return 2;
  }
  using namespace colate_drv;
  int bad = 0;
  const std::string dir = argv[1], big_dir = dir + "/big";
  const std::vector<std::string> names = {"1", "2", "3"};
  const int kScale = 70000;
  ::mkdir(big_dir.c_str(), 0777);
  if (!write_inputs(dir, names, 300, TopoInputs{97531, false, true, 7, 1}) || !write_inputs(big_dir, names, 300, TopoInputs{97531, false, true, 7, kScale})) {
    std::fprintf(stderr, "cannot write the inputs under %s\n", dir.c_str());
    return 1;
  }
  std::vector<std::string> mut_files, big_mut_files;
  for (const std::string& c : names) mut_files.push_back(dir + "/P_chr" + c + ".mut"), big_mut_files.push_back(big_dir + "/P_chr" + c + ".mut");
  const std::vector<PairSpec> triples = triples_of(dir), big_triples = triples_of(big_dir);
  const int P = (int)triples.size(), C = (int)names.size();

  WalkInputs in, big;
  if (!load_walk_inputs(names, mut_files, triples, in, RowSet::count_topo) || !in.indexed || !in.files_ok || in.S != 4 || (int)in.cond_ids.size() != P ||
      in.cidx_ptrs.size() != (size_t)in.S * C) {
    std::fprintf(stderr, "the inputs were not indexed (%d samples)\n", in.S);
    return 1;
  }
  if (!load_walk_inputs(names, big_mut_files, big_triples, big, RowSet::count_topo) || big.indexed || !big.files_ok) {
    std::fprintf(stderr, "the inputs with counts beyond 16 bits were indexed, or not read\n");
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
  colate_topo::View v;
  v.C = C, v.row_off = in.row_off.data(), v.rows = in.row_ptrs.data(), v.S = in.S, v.idx = in.idx_ptrs.data(), v.cidx = in.cidx_ptrs.data();
  v.P = P, v.triples = ids.data();

  long long qualifying = 0, fractional = 0, whole = 0;
  for (const std::vector<double>& ep : epoch_sets)
    for (int nbpb : {30000000, 100000, 7001}) {
      const int E = (int)ep.size();
      if (E == colate_topo::kMaxProfileEpochs && nbpb == 7001) continue;  // (300 blocks x 1024 epochs x 7 triples say nothing the others do not)
      std::vector<int> blk_off, big_off;
      if (topo_cursor_blocks(in, nbpb, blk_off) || topo_cursor_blocks(big, nbpb, big_off) || blk_off != big_off) return std::fprintf(stderr, "blocks\n"), 1;
      const int nb = blk_off[(size_t)C];
      const size_t per_block = (size_t)E * 3;
      TopoProfile want, want_big, sampled;
      for (TopoProfile* t : {&want, &want_big, &sampled}) t->E = E, t->epochs = ep.data(), t->nbpb = nbpb, t->blk_off = blk_off.data();
      if (!topo_cursor_expected(in, names, triples, want) || !topo_cursor_expected(big, names, big_triples, want_big)) return 1;
      std::vector<std::vector<TopoLine>> lines;
      std::vector<long long> draws;
      if (!topo_cursor_triples(in, names, triples, 78, lines, draws, &sampled)) return 1;
      bad += want.blocks.size() != (size_t)P * nb * per_block || want.counts.size() != (size_t)P * per_block;
      if (want_big.blocks != want.blocks || want_big.counts != want.counts) {
        std::fprintf(stderr, "E = %d, %d bases per block: the counts times %d give other integers\n", E, nbpb, kScale);
        bad++;
      }
      for (int p = 0; p < P; p++) {
        std::vector<long long> sum(per_block, 0);
        for (int b = 0; b < nb; b++)
          for (size_t k = 0; k < per_block; k++) sum[k] += want.blocks[((size_t)p * nb + b) * per_block + k];
        for (size_t k = 0; k < per_block; k++) bad += sum[k] != want.counts[(size_t)p * per_block + k];
        long long rows_in = 0;
        for (size_t k = 0; k < (size_t)nb * E; k++) {
          const long long* const x = &want.blocks[((size_t)p * nb * E + k) * 3];
          bad += x[0] < 0 || x[1] < 0 || x[0] + x[1] > x[2] * colate_topo::kExpectedOne;
          bad += x[2] != sampled.blocks[((size_t)p * nb * E + k) * 3 + 2];  // the qualifying rows are those of the sampled walk
          rows_in += x[2];
          if (nbpb == 7001 && E == 1) (x[0] % colate_topo::kExpectedOne || x[1] % colate_topo::kExpectedOne ? fractional : whole) += x[2] > 0;
        }
        bad += rows_in != draws[(size_t)p];
        if (E == 1 && nbpb == 7001) qualifying += rows_in;
      }
      for (int form = 0; form < 2; form++) {
        std::vector<long long> counts((size_t)P * nb * per_block, -1);
        const int rc = form == 0 ? colate_topo::topo_expected_blocks_host(v, E, ep.data(), nbpb, nb, counts.data())
                                 : colate_topo_expected_blocks_host(C, in.row_off.data(), in.rows.data(), in.S, idx.data(), cidx.data(), P, ids.data(), E,
                                                                    ep.data(), nbpb, nb, counts.data());
        if (rc) {
          std::fprintf(stderr, "expected blocks host form %d: %d (%s)\n", form, rc, colate_last_error());
          return 1;
        }
        if (counts != want.blocks) {
          std::fprintf(stderr, "E = %d, %d bases per block, form %d: the counts differ from the cursor walk's\n", E, nbpb, form);
          bad++;
        }
      }
    }
  bad += qualifying < 300 || fractional < 20 || whole < 20;  // (cells with a fractional expectation and cells of fixed rows alone)

  // ---- the addends at the edges of 16 and 32 bits against a 128-bit quotient; scaled counts give the quotients of the small ones
  {
    const unsigned long long edge[] = {0, 1, 2, 32767, 65534, 65535, 65536, 65537, 0x7fffffffull, 0xfffffffeull, 0xffffffffull};
    for (unsigned long long a : edge)
      for (unsigned long long b : edge)
        for (unsigned long long c : edge)
          for (unsigned long long d : edge) {
            if (a + b == 0 || c + d == 0) continue;
            const colate_topo::Addends x = colate_topo::expected_addends(a, b, c, d);
            const unsigned __int128 den = (unsigned __int128)(a + b) * (c + d);
            bad += x.plus != (unsigned long long)((((unsigned __int128)a * d) << 30) / den) ||
                   x.minus != (unsigned long long)((((unsigned __int128)b * c) << 30) / den) || x.plus + x.minus > (1ull << 30);
            if ((a | b | c | d) < 60000) {
              const colate_topo::Addends y = colate_topo::expected_addends(a * kScale, b * kScale, c * kScale, d * kScale);
              bad += y.plus != x.plus || y.minus != x.minus;
            }
          }
    const colate_topo::Addends fixed = colate_topo::expected_addends(7, 0, 0, 3), none = colate_topo::expected_addends(7, 0, 5, 0);
    bad += fixed.plus != (1ull << 30) || fixed.minus != 0 || none.plus != 0 || none.minus != 0;
  }

  // ---- refusals: the code, the name, nothing written
  const std::vector<double>& ep = epoch_sets[0];
  std::vector<int> blk_off;
  if (topo_cursor_blocks(in, 100000, blk_off)) return 1;
  const int nb = blk_off[(size_t)C];
  auto refused = [&](const char* what, int code, int E, const double* epochs, int nbpb, int nb_given, bool with_counts, bool device = false,
                     const colate_topo::Triple* tr = nullptr) {
    std::vector<long long> counts((size_t)P * ((size_t)nb + 1) * 64 * 3, -7);
    const int rc = (device ? colate_topo_expected_blocks : colate_topo_expected_blocks_host)(
        C, in.row_off.data(), in.rows.data(), in.S, idx.data(), cidx.data(), P, tr ? tr : ids.data(), E, epochs, nbpb, nb_given,
        with_counts ? counts.data() : nullptr);
    bool untouched = true;
    for (long long x : counts) untouched = untouched && x == -7;
    if (rc != code || !std::strstr(colate_last_error(), what) || !untouched) {
      std::fprintf(stderr, "refusal `%s`: rc %d, message `%s`, outputs %s\n", what, rc, colate_last_error(), untouched ? "untouched" : "written");
      bad++;
    }
  };
  refused("E = 0 epochs", COLATE_EINVAL, 0, ep.data(), 100000, nb, true);
  std::vector<double> e2 = ep;
  e2[3] = e2[2];
  refused("epochs[3]", COLATE_EINVAL, E0, e2.data(), 100000, nb, true);
  refused("NULL pointer", COLATE_EINVAL, E0, nullptr, 100000, nb, true);
  refused("NULL pointer", COLATE_EINVAL, E0, ep.data(), 100000, nb, false);
  refused("num_bases_per_block = 0", COLATE_EINVAL, E0, ep.data(), 0, nb, true);
  refused("at or above 2^31 - num_bases_per_block", COLATE_EINVAL, E0, ep.data(), 2147483647, 3, true);
  refused("(needed: ", COLATE_ELIMIT, E0, ep.data(), 13, nb, true);
  refused("is not the", COLATE_EINVAL, E0, ep.data(), 100000, nb + 1, true);
  refused("is not the", COLATE_EINVAL, E0, ep.data(), 100000, nb - 1, true);
  std::vector<colate_topo::Triple> out_of_range = ids;
  out_of_range[2].reference = in.S;
  refused("triple 2: sample id out of range", COLATE_EINVAL, E0, ep.data(), 100000, nb, true, false, out_of_range.data());
  refused("no device", COLATE_ENODEVICE, E0, ep.data(), 100000, nb, true, true);

  std::printf("%d triples over %d samples, %lld rows, %lld qualifying rows, %lld cells with a fractional expectation and %lld without at 7001 bases per block\n",
              P, in.S, nrows, qualifying, fractional, whole);
  if (bad) {
    std::fprintf(stderr, "%d mismatches\n", bad);
    return 1;
  }
  std::printf("ok\n");
  return 0;
}
