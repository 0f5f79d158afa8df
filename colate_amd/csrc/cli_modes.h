// colate_amd/csrc/cli_modes.h -- the modes of `Colate` as colate_mut_main's table calls them, one entry point per driver file.
#pragma once
#include "cli_options.h"

namespace colate_drv {

int run_mut(const Options& opt);            // mut_driver.cpp: one pair
int run_mut_pairs(const Options& opt);      // mut_driver.cpp: `--pairs LIST` (both are what a rank of `--ranks` runs)
int run_mut_interval(const Options& opt);   // mut_interval.cpp
int run_compare_tmp(const Options& opt);    // compare_driver.cpp
int run_count_topo(const Options& opt);     // topo_driver.cpp
int run_make_tmp(const Options& opt);       // make_tmp.cpp
int run_condcoal(const Options& opt);       // condcoal.cpp: `--mode CondCoalRates`

}  // namespace colate_drv
