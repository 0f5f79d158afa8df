// colate_amd/csrc/tools/no_device_stubs.cpp -- ONLY for the host sanitizer binary (`make asan` -> bin/Colate_asan):
// the host side of the library (mut_host.cpp, mut_driver.cpp) built with g++ -fsanitize=address,undefined, without
// HIP.  Every compute entry point that needs a device is defined here to FAIL with COLATE_ENODEVICE -- the sanitizer
// runs cover the readers, the table fill, the bootstrap, make_tmp and the writers (--counts_only); nothing here
// computes anything, and libcolate_amd.so does not contain this file.
#include <cstdarg>
#include <cstdio>
#include <string>

#include "colate_amd.h"
#include "colate_internal.h"
#include "em_build.hpp"

namespace colate {
static thread_local std::string g_err;
int fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}
void mark_device_touched() {}  // (no runtime to bring up: colate_device_touched() stays 0)
ProfRange::ProfRange(const char*) {}
ProfRange::~ProfRange() {}
}  // namespace colate

static int nodev() { return colate::fail(COLATE_ENODEVICE, "host sanitizer build: no device code linked"); }

extern "C" {
const char* colate_version(void) { return "colate_amd host sanitizer build (no device code)"; }
const char* colate_last_error(void) { return colate::g_err.c_str(); }
int colate_device_touched(void) { return 0; }
int colate_device_count(void) { return nodev(); }
int colate_set_device(int) { return nodev(); }
int colate_warm_up(int) { return nodev(); }
int colate_em_force_variant(int) { return nodev(); }
int colate_em_kernel_build(int, int, char*, int) { return nodev(); }
// (the dispatch table needs no device: em_build.hpp's own answers, as in the library)
static int build_name_result(int rc) { return rc >= 0 ? rc : colate::fail(COLATE_EINVAL, "%s", kEmBuildErrors[-rc]); }
int colate_em_kernel_build_for(int mode, int B, int E, int cus, int forced, char* name, int cap) {
  return build_name_result(em_build_name_for(mode, B, E, cus, forced, name, cap));
}
int colate_em_kernel_builds(int mode, char* buf, int cap) { return build_name_result(em_build_names(mode, buf, cap)); }
int colate_em_batch(int, int, int, const double*, const double*, const double*, const double*, const double*, int, int,
                    double, double, double*, int*, double*, int*) { return nodev(); }
int colate_em_batch_rows(int, int, int, const double*, const double*, const double*, const double*, const double*, int, int,
                         double, double, double*, int*, double*, int*) { return nodev(); }
int colate_em_batch_sharded(int, const int*, int, int, int, const double*, const double*, const double*, const double*,
                            const double*, int, int, double, double, double*, int*, double*, int*) { return nodev(); }
int colate_em_batch_rows_sharded(int, const int*, int, int, int, const double*, const double*, const double*, const double*,
                                 const double*, int, int, double, double, double*, int*, double*, int*) { return nodev(); }
int colate_bootstrap_em_batch_sharded(int, const int*, int, int, int, int, const double*, double, const double*, const double*,
                                      const double*, const double*, const double*, const double*, const double*, int, int, double,
                                      double, double*, int*, double*, int*, double*, double*) { return nodev(); }
int colate_bootstrap_em_batch_groups_sharded(int, const int*, int, int, int, int, const double*, const int*, const double*,
                                             const double*, const double*, const double*, const double*, const double*,
                                             const double*, const double*, int, int, double, double, double*, int*, double*, int*,
                                             double*, double*) { return nodev(); }
int colate_bootstrap_em_batch(int, int, int, int, const double*, double, const double*, const double*, const double*,
                              const double*, const double*, const double*, const double*, int, int, double, double, double*,
                              int*, double*, int*, double*, double*) { return nodev(); }
int colate_bootstrap_em_interval_batch(int, int, int, int, const int*, const double*, const double*, const double*, const double*,
                                       const double*, const double*, int, int, double, double, double*, int*, double*, int*) {
  return nodev();
}
int colate_interval_cells(long long, const colate_interval_rec*, const int*, int, int, int*, double*, double*, double*, long long*) {
  return nodev();
}
int colate_interval_fit_groups(int, int, int, const long long*, const colate_interval_rec*, const int*, const int*, const double*,
                               const double*, const double*, int, int, double, double, int*, long long*, double*, int*, double*,
                               int*) {
  return nodev();
}
double colate_interval_fit_groups_kernel_seconds(void) { return 0.0; }
double colate_interval_fit_samples_kernel_seconds(void) { return 0.0; }
int colate_shard_bounds(int B, int nranks, int rank, int* lo, int* hi) {
  const int base = B / nranks, rem = B % nranks;
  *lo = rank * base + (rank < rem ? rank : rem);
  *hi = *lo + base + (rank < rem ? 1 : 0);
  return COLATE_OK;
}
int colate_bootstrap_em_batch_groups(int, int, int, int, const double*, const int*, const double*, const double*, const double*,
                                     const double*, const double*, const double*, const double*, const double*, int, int, double,
                                     double, double*, int*, double*, int*, double*, double*) { return nodev(); }
int colate_bootstrap_em_batch_groups_allgather(void*, int, int, int, int, int, int, const double*, const int*, const double*,
                                               const double*, const double*, const double*, const double*, const double*,
                                               const double*, const double*, int, int, double, double, double*, int*, double*,
                                               int*) { return nodev(); }
int colate_comm_unique_id(void*) { return nodev(); }
int colate_comm_create(const void*, int, int, void**) { return nodev(); }
int colate_comm_destroy(void*) { return COLATE_OK; }
int colate_em_batch_allgather(void*, int, int, int, const double*, const double*, const double*, const double*, const double*,
                              int, int, double, double, double*, int*, double*, int*) { return nodev(); }
int colate_bootstrap_em_batch_allgather(void*, int, int, int, int, const double*, double, const double*, const double*,
                                        const double*, const double*, const double*, const double*, const double*, int, int,
                                        double, double, double*, int*, double*, int*) { return nodev(); }
}

// the pair walk on the device (interval_walk.h; colate_interval_walk and colate_interval_fit_samples end here): none in this build
#include "interval_walk.h"
namespace colate_iw {
int walk_view_device(const View&, long long, long long*, int*, colate_ic::IntervalRec*, int*) { return nodev(); }
int fit_samples_view_device(const View&, const FitArgs&) { return nodev(); }
}  // namespace colate_iw

// the table fill over walk indices on the device (fill_samples.h; colate_fill_samples ends here): none in this build
#include "fill_samples.h"
namespace colate_fs {
int fill_view_device(const colate_iw::View&, int, unsigned, Result&) { return nodev(); }
}  // namespace colate_fs

// the pair stage of `--mode compare_tmp` on the device (compare_tmp.h; colate_compare_samples ends here): none in this build
#include "compare_tmp.h"
namespace colate_cmp {
int compare_view_device(const View&, long long, long long*, int*, int*) { return nodev(); }
}  // namespace colate_cmp
// the triple stage of `--mode count_topo` on the device (count_topo.h; colate_topo_samples ends here): none in this build
#include "count_topo.h"
namespace colate_topo {
int topo_view_device(const View&, long long, long long*, unsigned long long*, unsigned long long*, long long*) { return nodev(); }
int topo_profile_device(const View&, int, const double*, long long*, long long*) { return nodev(); }
int topo_profile_blocks_device(const View&, int, const double*, int, int, long long*, long long*) { return nodev(); }
int topo_expected_blocks_device(const View&, int, const double*, int, int, long long*) { return nodev(); }
}  // namespace colate_topo
extern "C" {
int colate_compare_samples_chunks(void) { return 0; }
double colate_compare_samples_kernel_seconds(void) { return 0.0; }
int colate_topo_samples_chunks(void) { return 0; }
double colate_topo_samples_kernel_seconds(void) { return 0.0; }
int colate_topo_profile_chunks(void) { return 0; }
double colate_topo_profile_kernel_seconds(void) { return 0.0; }
int colate_topo_profile_blocks_chunks(void) { return 0; }
double colate_topo_profile_blocks_kernel_seconds(void) { return 0.0; }
int colate_topo_expected_blocks_chunks(void) { return 0; }
double colate_topo_expected_blocks_kernel_seconds(void) { return 0.0; }
}

// the age sampling on the device (fill_device.h): there is none in this build, the host code samples
#include "fill_device.h"
namespace colate_drv {
bool fill_device_available() { return false; }
std::unique_ptr<DeviceFill> make_device_fill(int, int, const double*, const double*, size_t, size_t, std::string& why) {
  why = "built without a device";
  return nullptr;
}
}  // namespace colate_drv

// the CondCoalRates walks on the device (condcoal.h): none in this build, the host twin walks
#include "condcoal.h"
namespace colate_cc {
std::unique_ptr<CcWalker> make_device_walker(int, const CcRun&, int, std::string& why) {
  why = "built without a device";
  return nullptr;
}
std::unique_ptr<CcWalker> make_pairs_device_walker(int, const CcRun&, const std::vector<int>&, const std::vector<int>&, int,
                                                   std::string& why) {
  why = "built without a device";
  return nullptr;
}
}  // namespace colate_cc

// the pair counting of CoalRate on the device (coalrate.h): none in this build, the host twin counts
#include "coalrate.h"
namespace colate_cr {
std::unique_ptr<CoalRateWalker> make_device_walker(int, const CrRun&, const CrTables&, int, std::string& why, int*) {
  why = "built without a device";
  return nullptr;
}
}  // namespace colate_cr

// the per-tree sort of CoalRate --mode tree on the device (coalrate_tree.h): none in this build, the host twin sorts
#include "coalrate_tree.h"
namespace colate_crt {
std::unique_ptr<CoalTreeWalker> make_device_walker(int, int, const std::vector<double>&, int, std::string& why, int*) {
  why = "built without a device";
  return nullptr;
}
}  // namespace colate_crt
