// colate_amd/csrc/coalrate_cli.cpp -- the `CoalRate` executable of colate_amd: the reference's command line for
// `--mode local_ancestry` (include/coal/CoalRate.cpp), implemented in libcolate_amd.so (colate_coalrate_main).
#include "colate_amd.h"

int main(int argc, char** argv) { return colate_coalrate_main(argc, argv); }
