// colate_amd/csrc/mut_interval.h -- `Colate --mode mut_interval`: the rows file of interval-dated observations per genome
// block -- or the SNPs a pair uses, through colate_interval_cells -- and the driver around colate_bootstrap_em_interval_batch
// (mut_interval.cpp; its entry point: cli_modes.h); with --pairs, the driver around colate_interval_fit_groups.
#pragma once
#include <string>
#include <vector>

namespace colate_drv {

// What a rows file becomes.  Lines `block kind age_begin age_end weight`; distinct block ids, ascending, are the table rows
// 0 .. nb-1, distinct (kind, age_begin, age_end) triples (equal as parsed doubles), in order of first appearance, the R
// rows; repeated lines of one cell add up in file order.
struct IntervalRows {
  int nb = 0, R = 0;
  std::vector<long long> block_ids;      // [nb] ascending
  std::vector<int> kinds;                // [R] 0 = shared, 1 = not shared (colate_em_interval_calls)
  std::vector<double> age_begin, age_end;  // [R] generations
  std::vector<double> tables;            // [nb][R]
};

// Reads `path` (plain or gzip).  Blank lines and lines starting with '#' are skipped; any other line that is not five
// fields -- a non-negative integer, `shared` / `notshared`, two finite ages with epoch0 <= age_begin <= age_end (what
// colate_em_interval_calls accepts for epochs[0] = epoch0), a finite weight >= 0 -- is an error: false, and `err` names
// the file and the line number.  A file without rows is an error as well.
bool read_interval_rows(const std::string& path, double epoch0, IntervalRows& out, std::string& err);

}  // namespace colate_drv
