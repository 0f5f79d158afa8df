// colate_amd/csrc/colate_api.cpp -- extern "C" entry points of libcolate_amd.so
// for the EM hot path (see include/colate_amd.h).  Argument checking, device
// buffers for the host-pointer variants, kernel launch.  No CPU fallback.
#include <hip/hip_runtime.h>

#include <dlfcn.h>
#include <unistd.h>

#include <atomic>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "colate_amd.h"
#include "colate_internal.h"
#include "em_build.hpp"
#include "em_job.hpp"
#include "em_kernels.h"
#include "interval_cells.h"

static_assert(COLATE_FLAG_NAN == 1 && COLATE_FLAG_NEG == 2 && COLATE_FLAG_MAXITER == 4 && COLATE_FLAG_UNRESOLVED == 8 &&
                  COLATE_UNRESOLVED_SHIFT == 8, "flags");

namespace colate {

static thread_local std::string g_last_error;

int fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_last_error = buf;
  return code;
}

int hip_fail(hipError_t e, const char* what) {
  return fail(e == hipErrorNoDevice || e == hipErrorInvalidDevice ? COLATE_ENODEVICE : COLATE_EHIP,
              "%s: %s", what, hipGetErrorString(e));
}

static int check_sizes(int B, int E, int A) {
  if (B < 0 || E < 1 || A < 1) return fail(COLATE_EINVAL, "bad sizes B=%d E=%d A=%d", B, E, A);
  if (E > COLATE_EM_MAX_E || A > COLATE_EM_MAX_A)
    return fail(COLATE_ELIMIT, "E=%d / A=%d above compiled limits (%d / %d)", E, A,
                COLATE_EM_MAX_E, COLATE_EM_MAX_A);
  return COLATE_OK;
}

// ---- profiler ranges (roctx), bound on first use
namespace {
struct Roctx {
  int (*push)(const char*) = nullptr;
  int (*pop)() = nullptr;
};
const Roctx& roctx() {
  static const Roctx r = [] {
    Roctx x;
    if (!std::getenv("COLATE_ROCTX")) return x;  // (opt-in: COLATE_ROCTX=1 under `rocprofv3 --marker-trace`; otherwise no profiler library is loaded)
    for (const char* name : {"librocprofiler-sdk-roctx.so.1", "libroctx64.so.4", "librocprofiler-sdk-roctx.so", "libroctx64.so"}) {
      if (void* h = dlopen(name, RTLD_NOW | RTLD_LOCAL)) {
        x.push = reinterpret_cast<int (*)(const char*)>(dlsym(h, "roctxRangePushA"));
        x.pop = reinterpret_cast<int (*)()>(dlsym(h, "roctxRangePop"));
        if (x.push && x.pop) break;
        x.push = nullptr, x.pop = nullptr;
      }
    }
    return x;
  }();
  return r;
}
}  // namespace
ProfRange::ProfRange(const char* name) {
  if (roctx().push) roctx().push(name);
}
ProfRange::~ProfRange() {
  if (roctx().pop) roctx().pop();
}

static std::atomic<int> g_device_touched{0};
void mark_device_touched() { g_device_touched.store(1, std::memory_order_relaxed); }

int ensure_device() {
  mark_device_touched();
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess || n <= 0)
    return fail(COLATE_ENODEVICE, "no usable HIP device (%s); libcolate_amd has no CPU fallback",
                e == hipSuccess ? "device count 0" : hipGetErrorString(e));
  return COLATE_OK;
}

// grids that the kernel's contiguous-segment logic relies on
int check_grids(int E, int A, const double* age_grid, const double* epochs) {
  for (int b = 0; b < A; b++) {
    if (!(age_grid[b] >= 0.0) || (b > 0 && age_grid[b] < age_grid[b - 1]))
      return fail(COLATE_EINVAL, "age_grid must be non-negative and non-decreasing (index %d)", b);
  }
  for (int e = 1; e < E; e++) {
    if (!(epochs[e] >= epochs[e - 1]))
      return fail(COLATE_EINVAL, "epochs must be non-decreasing (index %d)", e);
  }
  if (!(epochs[0] <= age_grid[0]))
    return fail(COLATE_EINVAL, "epochs[0] must not exceed age_grid[0]");
  return COLATE_OK;
}

// ---- staging arena of the host-pointer entry points (em_job.hpp) -------------------------------------
// One device buffer, one pinned host staging buffer and one stream per store, grown on demand and kept: a call costs
// one staged host-to-device copy, the launch(es), one device-to-host copy and one stream synchronisation instead of
// a hipMalloc/hipFree and a synchronous copy per array.
static std::atomic<int> g_process_exiting{0};

void ArenaStore::release() {
  if (device >= 0) {
    int cur = -1;
    (void)hipGetDevice(&cur);
    if (cur != device) (void)hipSetDevice(device);
    if (stream) (void)hipStreamDestroy(stream);
    if (d) (void)hipFree(d);
    if (h) (void)hipHostFree(h);
    if (cur >= 0 && cur != device) (void)hipSetDevice(cur);
  }
  *this = ArenaStore();
}

int ArenaStore::reserve(size_t dbytes, size_t hbytes) {
  int cur = 0;
  HIP_TRY(hipGetDevice(&cur));
  if (cur != device) {  // the thread moved to another GPU: start over there
    release();
    device = cur;
  }
  if (!stream) {
    static std::atomic<int> registered{0};  // (behind HIP's own exit handlers in the list, so it runs before them)
    if (!registered.exchange(1)) std::atexit([] { g_process_exiting.store(1); });
    HIP_TRY(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
  }
  if (dbytes > dcap) {
    if (d) (void)hipFree(d);
    d = nullptr, dcap = 0;
    const size_t want = dbytes + dbytes / 4 + 4096;
    HIP_TRY(hipMalloc(reinterpret_cast<void**>(&d), want));
    dcap = want;
  }
  if (hbytes > hcap) {
    if (h) (void)hipHostFree(h);
    h = nullptr, hcap = 0;
    const size_t want = hbytes + hbytes / 4 + 4096;
    HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&h), want, hipHostMallocDefault));
    hcap = want;
  }
  return COLATE_OK;
}

// The per-thread workspace: the store of the calls that run on the calling thread's device, kept between calls
// (colate_release_workspace frees it).  A thread that ends while the process lives frees its workspace (thread_local
// destructor below); the main thread's and whatever is left at process exit are not touched (a destructor there
// could run after the HIP runtime has shut down; the driver reclaims everything anyway).
struct WorkspaceOwner {
  ArenaStore ws;
  ~WorkspaceOwner() {  // a short-lived worker thread must not leak HBM, pinned memory and a stream per thread
    const bool main_thread = (::getpid() == (pid_t)::gettid());
    if (!main_thread && !g_process_exiting.load()) ws.release();
  }
};
static thread_local WorkspaceOwner g_ws_owner;
ArenaStore& thread_workspace() { return g_ws_owner.ws; }

int Arena::commit() {
  auto round_up = [](size_t b) { return (b + 255) & ~size_t(255); };
  size_t sizes[3] = {0, 0, 0};
  for (Seg& s : seg_) {
    s.koff = sizes[s.kind];
    sizes[s.kind] += round_up(s.bytes);
  }
  const size_t base[3] = {0, sizes[kIn], sizes[kIn] + sizes[kScratch]};  // device: in | scratch | out
  for (Seg& s : seg_) s.doff = base[s.kind] + s.koff;
  in_bytes_ = sizes[kIn], out_bytes_ = sizes[kOut], out_base_ = base[kOut];
  if (int rc = st_->reserve(base[kOut] + sizes[kOut], sizes[kIn] + sizes[kOut])) return rc;  // host: in | out
  committed_ = true;
  for (const Seg& s : seg_)
    if (s.kind == kIn && s.bytes) std::memcpy(st_->h + s.koff, s.src, s.bytes);
  if (in_bytes_) HIP_TRY(hipMemcpyAsync(st_->d, st_->h, in_bytes_, hipMemcpyHostToDevice, st_->stream));
  return COLATE_OK;
}

int Arena::finish() {
  if (!committed_) return COLATE_OK;
  char* hout = st_->h + in_bytes_;
  if (out_bytes_) HIP_TRY(hipMemcpyAsync(hout, st_->d + out_base_, out_bytes_, hipMemcpyDeviceToHost, st_->stream));
  HIP_TRY(hipStreamSynchronize(st_->stream));
  for (const Seg& s : seg_)
    if (s.kind == kOut && s.dst && s.bytes) std::memcpy(s.dst, hout + s.koff, s.bytes);
  return COLATE_OK;
}

static int launch(const ColateEmArgs& a, hipStream_t s) {
  mark_device_touched();
  if (a.B == 0) return COLATE_OK;
  hipError_t e = colate_em_launch(a, s);
  if (e != hipSuccess) return hip_fail(e, "EM kernel launch");
  return COLATE_OK;
}

// colate_em_batch_device, plus the log-likelihood trace ([B][ll_trace_cap] on the device, or NULL)
static int em_batch_device(int B, int E, int A, const double* age_grid, const double* cnt_shared,
                           const double* cnt_notshared, const double* epochs, int epochs_per_replicate,
                           const double* init_rates, int rates_per_replicate, int max_iter, int min_iter,
                           double rel_tol, double rate_floor, double* out_rates, int* out_iters, double* out_loglik,
                           int* out_flags, double* ll_trace, int ll_trace_cap, hipStream_t stream) {
  if (int rc = check_sizes(B, E, A)) return rc;
  if (!age_grid || !cnt_shared || !cnt_notshared || !epochs || !init_rates || !out_rates ||
      !out_iters || !out_loglik || !out_flags)
    return fail(COLATE_EINVAL, "NULL pointer argument");
  if (max_iter < 1) return fail(COLATE_EINVAL, "max_iter must be >= 1");
  ColateEmArgs a{};
  a.B = B, a.E = E, a.A = A, a.mode = 0;
  a.age_grid = age_grid, a.cnt_sh = cnt_shared, a.cnt_ns = cnt_notshared;
  a.epochs = epochs, a.epochs_stride = epochs_per_replicate ? E : 0;
  a.rates_in = init_rates, a.rates_stride = rates_per_replicate ? E : 0;
  a.max_iter = max_iter, a.min_iter = min_iter, a.rel_tol = rel_tol, a.rate_floor = rate_floor;
  a.out_rates = out_rates, a.out_iters = out_iters, a.out_ll = out_loglik, a.out_flags = out_flags;
  a.ll_trace = ll_trace, a.ll_trace_cap = ll_trace_cap;
  return launch(a, stream);
}

int check_call(const EmJob& j) {
  if (int rc = check_sizes(j.R, j.E, j.A)) return rc;
  if (j.source == EmJob::kGenome && (j.nb < 1 || j.A < 2)) return fail(COLATE_EINVAL, "bad sizes nb=%d A=%d", j.nb, j.A);
  if (j.source == EmJob::kGroups && j.A < 2) return fail(COLATE_EINVAL, "bad sizes A=%d", j.A);
  if (!j.age_grid || !j.out_rates || !j.out_iters || !j.out_loglik || !j.out_flags)
    return fail(COLATE_EINVAL, "NULL pointer argument");
  if (j.max_iter < 1) return fail(COLATE_EINVAL, "max_iter must be >= 1");
  return COLATE_OK;
}

int check_inputs(const EmJob& j) {
  const bool groups = j.source == EmJob::kGroups;
  bool null = !j.epochs || !j.init_rates;
  if (j.source == EmJob::kTables) null = null || !j.cnt_shared || !j.cnt_notshared;
  else null = null || !j.weights || !j.block[0] || !j.block[1] || !j.block[2] || !j.block[3];
  if (groups) null = null || !j.group_nb || !j.group_age;
  if (null) return fail(COLATE_EINVAL, "NULL pointer argument");
  for (int g = 0; groups && g < j.group_count; g++)
    if (j.group_nb[g] < 1) return fail(COLATE_EINVAL, "group %d has %d genome blocks", j.group_first + g, j.group_nb[g]);
  const int epoch_rows = j.layout == EmJob::kShared ? 1 : j.layout == EmJob::kPerRow ? j.R : j.group_count;
  for (int b = 0; b < epoch_rows; b++)
    if (int rc = check_grids(j.E, j.A, j.age_grid, j.epochs + (size_t)b * j.E)) return rc;
  return COLATE_OK;
}

int enqueue_rows(const EmJob& j, int lo, int hi, Arena& ar, int* status, RowOut out) {
  const int n = hi - lo, E = j.E, A = j.A;
  const size_t nA = (size_t)n * A, nE = (size_t)n * E;
  const int i_grid = ar.in(j.age_grid, A);
  // epochs and starting rates: shared, or one row per row (the EM kernel's per-replicate layout)
  const bool per_row = j.layout != EmJob::kShared;
  const double *ep = j.epochs, *init = j.init_rates;
  std::vector<double> row_ep, row_init;
  if (j.layout == EmJob::kPerRow) ep += (size_t)lo * E, init += (size_t)lo * E;
  if (j.layout == EmJob::kPerGroup) {
    row_ep.resize(nE), row_init.resize(nE);
    expand_group_rows(j.epochs, j.B, j.group_first, lo, hi, E, row_ep.data());
    expand_group_rows(j.init_rates, j.B, j.group_first, lo, hi, E, row_init.data());
    ep = row_ep.data(), init = row_init.data();
  }
  const int i_ep = ar.in(ep, per_row ? nE : (size_t)E), i_init = ar.in(init, per_row ? nE : (size_t)E);
  // counts: the rows' slice of the given tables, or made on the device by a bootstrap kernel; those stay there
  // between the two kernels and travel back only if asked for
  int c_sh, c_ns, o_status = -1, i_w = -1, i_t[4] = {-1, -1, -1, -1}, i_nb = -1, i_bo = -1, i_wo = -1, i_age = -1;
  int g0 = 0, ng = 0;  // kGroups: the rows' groups are [g0, g0 + ng) of the job's
  std::vector<long long> block_off, weight_off;
  if (j.source == EmJob::kTables) {
    c_sh = ar.in(j.cnt_shared + (size_t)lo * A, nA), c_ns = ar.in(j.cnt_notshared + (size_t)lo * A, nA);
  } else {
    auto counts = [&](double* host) {
      if (!j.out_cnt_shared && !j.out_cnt_notshared) return ar.scratch<double>(nA);
      return ar.out(host ? host + (size_t)lo * A : host, nA);
    };
    c_sh = counts(j.out_cnt_shared), c_ns = counts(j.out_cnt_notshared);
    o_status = ar.out(status, 1);  // device int the bootstrap kernel ORs into; read back with the outputs
    long long first_block = 0, nblocks = j.nb;
    size_t first_weight = (size_t)lo * j.nb, nweights = (size_t)n * j.nb;
    if (j.source == EmJob::kGroups) {
      g0 = lo / j.B - j.group_first, ng = (hi - 1) / j.B - lo / j.B + 1;
      for (int g = 0; g < g0; g++) first_block += j.group_nb[g];
      block_off.resize(ng), weight_off.resize(ng);
      nblocks = 0;
      for (int g = 0; g < ng; g++) {
        block_off[g] = nblocks, weight_off[g] = nblocks * j.B;
        nblocks += j.group_nb[g0 + g];
      }
      first_weight = (size_t)first_block * j.B, nweights = (size_t)nblocks * j.B;
      i_nb = ar.in(j.group_nb + g0, ng), i_age = ar.in(j.group_age + g0, ng);
      i_bo = ar.in(block_off.data(), ng), i_wo = ar.in(weight_off.data(), ng);
    }
    i_w = ar.in(j.weights + first_weight, nweights);
    for (int k = 0; k < 4; k++) i_t[k] = ar.in(j.block[k] + (size_t)first_block * A, (size_t)nblocks * A);
  }
  int o_rates = -1, o_ll = -1, o_iters = -1, o_flags = -1;
  if (!out.rates)
    o_rates = ar.out(j.out_rates + (size_t)lo * E, nE), o_ll = ar.out(j.out_loglik + lo, n),
    o_iters = ar.out(j.out_iters + lo, n), o_flags = ar.out(j.out_flags + lo, n);
  const size_t ntrace = j.ll_trace ? (size_t)n * j.ll_trace_cap : 0;
  const int o_trace = ntrace ? ar.out(j.ll_trace + (size_t)lo * j.ll_trace_cap, ntrace) : -1;
  if (int rc = ar.commit()) return rc;
  if (!out.rates) out = RowOut{ar.dev<double>(o_rates), ar.dev<double>(o_ll), ar.dev<int>(o_iters), ar.dev<int>(o_flags)};
  if (ntrace) HIP_TRY(hipMemsetAsync(ar.dev<double>(o_trace), 0xff, ntrace * sizeof(double), ar.stream()));  // NaN = "not reached"
  if (o_status >= 0) HIP_TRY(hipMemsetAsync(ar.dev<int>(o_status), 0, sizeof(int), ar.stream()));
  const double* grid = ar.dev<double>(i_grid);
  int rc = COLATE_OK;
  if (j.source == EmJob::kGenome)
    rc = colate_bootstrap_counts_device(n, j.nb, A, grid, j.age, ar.dev<double>(i_w), ar.dev<double>(i_t[0]),
                                        ar.dev<double>(i_t[1]), ar.dev<double>(i_t[2]), ar.dev<double>(i_t[3]),
                                        ar.dev<double>(c_sh), ar.dev<double>(c_ns), ar.dev<int>(o_status), ar.stream());
  if (j.source == EmJob::kGroups)
    rc = colate_bootstrap_counts_groups_device(ng, j.B, j.group_first + g0, lo, hi, A, grid, ar.dev<int>(i_nb),
                                               ar.dev<long long>(i_bo), ar.dev<long long>(i_wo), ar.dev<double>(i_age),
                                               ar.dev<double>(i_w), ar.dev<double>(i_t[0]), ar.dev<double>(i_t[1]),
                                               ar.dev<double>(i_t[2]), ar.dev<double>(i_t[3]), ar.dev<double>(c_sh),
                                               ar.dev<double>(c_ns), ar.dev<int>(o_status), ar.stream());
  if (rc) return rc;
  return em_batch_device(n, E, A, grid, ar.dev<double>(c_sh), ar.dev<double>(c_ns), ar.dev<double>(i_ep), per_row,
                         ar.dev<double>(i_init), per_row, j.max_iter, j.min_iter, j.rel_tol, j.rate_floor, out.rates,
                         out.iters, out.loglik, out.flags, ntrace ? ar.dev<double>(o_trace) : nullptr, j.ll_trace_cap,
                         ar.stream());
}

int finish_rows(Arena& arena, const int& status) {
  if (int rc = arena.finish()) return rc;
  if (status) return fail(COLATE_EINVAL, "sample age outside the age grid");
  return COLATE_OK;
}

// placement "this device": all rows on the calling thread's workspace
static int run_here(const EmJob& job, const char* range_name) {
  if (int rc = check(job)) return rc;
  if (int rc = ensure_device()) return rc;
  if (job.R == 0) return COLATE_OK;
  ProfRange range(range_name);
  Arena arena(thread_workspace());
  int status = 0;
  if (int rc = enqueue_rows(job, 0, job.R, arena, &status)) return rc;
  return finish_rows(arena, status);
}

// placement "devices list": contiguous shards of the rows, one per listed device, each on a store of its own
static int run_on_devices(const EmJob& job, int num_devices, const int* devices) {
  if (num_devices < 1 || !devices) return fail(COLATE_EINVAL, "need at least one device");
  if (int rc = check(job)) return rc;
  if (int rc = ensure_device()) return rc;
  int ndev_avail = 0;
  HIP_TRY(hipGetDeviceCount(&ndev_avail));
  for (int d = 0; d < num_devices; d++)
    if (devices[d] < 0 || devices[d] >= ndev_avail)
      return fail(COLATE_EINVAL, "device ordinal %d out of range (%d devices)", devices[d], ndev_avail);
  int prev_dev = 0;
  HIP_TRY(hipGetDevice(&prev_dev));
  struct Shard {
    ArenaStore store;
    Arena arena{store};
    int lo = 0, hi = 0, status = 0;
    bool launched = false;
  };
  std::vector<Shard> shards(num_devices);
  int rc = COLATE_OK;
  auto on_device = [&](int d) {
    const hipError_t e = hipSetDevice(devices[d]);
    if (e != hipSuccess && rc == COLATE_OK) rc = hip_fail(e, "hipSetDevice");
    return e == hipSuccess;
  };
  // Pass 1: per shard, stage, copy in and launch.  Nothing here waits for a device, so every GPU has its work queued
  // before the first result is asked for.
  for (int d = 0; d < num_devices && rc == COLATE_OK; d++) {
    Shard& s = shards[d];
    colate_shard_bounds(job.R, num_devices, d, &s.lo, &s.hi);
    if (s.hi == s.lo || !on_device(d)) continue;
    rc = enqueue_rows(job, s.lo, s.hi, s.arena, &s.status);
    s.launched = rc == COLATE_OK;
  }
  // Pass 2: collect.  A shard's copy-out waits for that shard's kernel only; the other GPUs keep running.
  for (int d = 0; d < num_devices && rc == COLATE_OK; d++)
    if (shards[d].launched && on_device(d)) rc = finish_rows(shards[d].arena, shards[d].status);
  for (Shard& s : shards) {  // always drain and release on the owning device, also after an error
    if (s.store.stream && hipSetDevice(s.store.device) == hipSuccess) (void)hipStreamSynchronize(s.store.stream);
    s.store.release();
  }
  (void)hipSetDevice(prev_dev);
  return rc;
}

}  // namespace colate

using namespace colate;

extern "C" {

const char* colate_version(void) { return "colate_amd 0.1 (gfx950)"; }
const char* colate_last_error(void) { return g_last_error.c_str(); }

int colate_device_touched(void) { return g_device_touched.load(std::memory_order_relaxed); }

int colate_device_count(void) {
  mark_device_touched();
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess) return fail(COLATE_ENODEVICE, "hipGetDeviceCount: %s", hipGetErrorString(e));
  return n;
}

int colate_set_device(int ordinal) {
  mark_device_touched();
  HIP_TRY(hipSetDevice(ordinal));
  return COLATE_OK;
}

int colate_warm_up(int ordinal) {
  // creates the HIP context of the device (a few hundred ms in a fresh process): a host that still has input files to
  // parse calls this from a second thread first (mut_driver.cpp)
  mark_device_touched();
  HIP_TRY(hipSetDevice(ordinal));
  HIP_TRY(hipFree(nullptr));
  return COLATE_OK;
}

int colate_em_kernel_variant(int B, int E) {
  if (B < 0 || E < 1 || E > COLATE_EM_MAX_E) return fail(COLATE_EINVAL, "bad sizes B=%d E=%d", B, E);
  if (int rc = ensure_device()) return rc;
  return colate_em_variant(B, E);
}

int colate_em_force_variant(int variant) {
  colate_em_set_forced_variant(variant);
  return COLATE_OK;
}

static int build_name_result(int rc) { return rc >= 0 ? rc : fail(COLATE_EINVAL, "%s", kEmBuildErrors[-rc]); }

int colate_em_kernel_build(int B, int E, char* name, int cap) {
  if (B < 0 || E < 1 || E > COLATE_EM_MAX_E) return fail(COLATE_EINVAL, "bad sizes B=%d E=%d", B, E);
  if (int rc = ensure_device()) return rc;
  return build_name_result(em_build_copy_name(colate_em_build(0, B, E), name, cap));
}

int colate_em_kernel_build_for(int mode, int B, int E, int cus, int forced, char* name, int cap) {
  return build_name_result(em_build_name_for(mode, B, E, cus, forced, name, cap));
}

int colate_em_kernel_builds(int mode, char* buf, int cap) { return build_name_result(em_build_names(mode, buf, cap)); }

int colate_em_batch_device(int B, int E, int A, const double* age_grid, const double* cnt_shared,
                           const double* cnt_notshared, const double* epochs, int epochs_per_replicate,
                           const double* init_rates, int rates_per_replicate, int max_iter, int min_iter,
                           double rel_tol, double rate_floor, double* out_rates, int* out_iters, double* out_loglik,
                           int* out_flags, void* hip_stream) {
  return em_batch_device(B, E, A, age_grid, cnt_shared, cnt_notshared, epochs, epochs_per_replicate, init_rates,
                         rates_per_replicate, max_iter, min_iter, rel_tol, rate_floor, out_rates, out_iters, out_loglik,
                         out_flags, nullptr, 0, static_cast<hipStream_t>(hip_stream));
}

int colate_em_estep_device(int B, int E, int A, const double* age_grid, const double* cnt_shared,
                           const double* cnt_notshared, const double* epochs, const double* rates, double* num_acc,
                           double* den_acc, double* loglik, int* flags, void* hip_stream) {
  if (int rc = check_sizes(B, E, A)) return rc;
  if (!age_grid || !cnt_shared || !cnt_notshared || !epochs || !rates || !num_acc || !den_acc ||
      !loglik || !flags)
    return fail(COLATE_EINVAL, "NULL pointer argument");
  ColateEmArgs a{};
  a.B = B, a.E = E, a.A = A, a.mode = 1;
  a.age_grid = age_grid, a.cnt_sh = cnt_shared, a.cnt_ns = cnt_notshared;
  a.epochs = epochs, a.epochs_stride = 0;
  a.rates_in = rates, a.rates_stride = E;
  a.max_iter = 1, a.min_iter = 0, a.rel_tol = 0, a.rate_floor = 0;
  a.out_ll = loglik, a.out_flags = flags, a.out_num = num_acc, a.out_den = den_acc;
  return launch(a, static_cast<hipStream_t>(hip_stream));
}

// colate_em_batch / colate_em_batch_rows: the job on this thread's workspace, plus the COLATE_LL_TRACE side output
static int em_batch_host(EmJob j) {
  // COLATE_LL_TRACE=<file>: the log-likelihood of every iteration (the reference's commented-out trace, coal.cpp:3659,
  // 3674, 3817, 3821), "replicate iteration loglik" per line.  Diagnostic: the run then takes the general loop with the
  // log-likelihood evaluated in every iteration (same rates, slower); at most the first kTraceCap iterations are kept.
  const char* trace_path = std::getenv("COLATE_LL_TRACE");
  constexpr int kTraceCap = 8192;
  const int cap = trace_path && j.R > 0 && j.max_iter > 0 ? (j.max_iter < kTraceCap ? j.max_iter : kTraceCap) : 0;
  std::vector<double> trace((size_t)(cap ? j.R : 0) * cap);
  if (cap) j.ll_trace = trace.data(), j.ll_trace_cap = cap;
  if (int rc = run_here(j, "colate_em_batch: H2D + EM kernel + D2H")) return rc;
  if (!cap) return COLATE_OK;
  FILE* f = std::fopen(trace_path, "w");
  if (!f) return fail(COLATE_EIO, "cannot write %s", trace_path);
  for (int b = 0; b < j.R; b++)
    for (int it = 0; it < cap; it++) {
      const double v = trace[(size_t)b * cap + it];
      if (v == v) std::fprintf(f, "%d %d %.17g\n", b, it, v);
    }
  std::fclose(f);
  return COLATE_OK;
}

int colate_em_batch(int B, int E, int A, const double* age_grid, const double* cnt_shared, const double* cnt_notshared,
                    const double* epochs, const double* init_rates, int max_iter, int min_iter, double rel_tol,
                    double rate_floor, double* out_rates, int* out_iters, double* out_loglik, int* out_flags) {
  return em_batch_host(tables_job(EmJob::kShared, B, E, A, age_grid, cnt_shared, cnt_notshared, epochs, init_rates,
                                  max_iter, min_iter, rel_tol, rate_floor, out_rates, out_iters, out_loglik, out_flags));
}

int colate_em_batch_rows(int B, int E, int A, const double* age_grid, const double* cnt_shared,
                         const double* cnt_notshared, const double* epochs, const double* init_rates, int max_iter,
                         int min_iter, double rel_tol, double rate_floor, double* out_rates, int* out_iters,
                         double* out_loglik, int* out_flags) {
  return em_batch_host(tables_job(EmJob::kPerRow, B, E, A, age_grid, cnt_shared, cnt_notshared, epochs, init_rates,
                                  max_iter, min_iter, rel_tol, rate_floor, out_rates, out_iters, out_loglik, out_flags));
}

int colate_em_batch_sharded(int num_devices, const int* devices, int B, int E, int A, const double* age_grid,
                            const double* cnt_shared, const double* cnt_notshared, const double* epochs,
                            const double* init_rates, int max_iter, int min_iter, double rel_tol, double rate_floor,
                            double* out_rates, int* out_iters, double* out_loglik, int* out_flags) {
  return run_on_devices(tables_job(EmJob::kShared, B, E, A, age_grid, cnt_shared, cnt_notshared, epochs, init_rates,
                                   max_iter, min_iter, rel_tol, rate_floor, out_rates, out_iters, out_loglik, out_flags),
                        num_devices, devices);
}

int colate_em_batch_rows_sharded(int num_devices, const int* devices, int B, int E, int A, const double* age_grid,
                                 const double* cnt_shared, const double* cnt_notshared, const double* epochs,
                                 const double* init_rates, int max_iter, int min_iter, double rel_tol,
                                 double rate_floor, double* out_rates, int* out_iters, double* out_loglik,
                                 int* out_flags) {
  return run_on_devices(tables_job(EmJob::kPerRow, B, E, A, age_grid, cnt_shared, cnt_notshared, epochs, init_rates,
                                   max_iter, min_iter, rel_tol, rate_floor, out_rates, out_iters, out_loglik, out_flags),
                        num_devices, devices);
}

int colate_bootstrap_em_batch_sharded(int num_devices, const int* devices, int B, int nb, int E, int A,
                                      const double* age_grid, double age, const double* weights,
                                      const double* sh_block, const double* ns_block, const double* sh_emp_block,
                                      const double* ns_emp_block, const double* epochs, const double* init_rates,
                                      int max_iter, int min_iter, double rel_tol, double rate_floor,
                                      double* out_rates, int* out_iters, double* out_loglik, int* out_flags,
                                      double* out_cnt_shared, double* out_cnt_notshared) {
  EmJob j = genome_job(B, nb, E, A, age_grid, age, weights, sh_block, ns_block, sh_emp_block, ns_emp_block, epochs,
                       init_rates, max_iter, min_iter, rel_tol, rate_floor, out_rates, out_iters, out_loglik, out_flags);
  j.out_cnt_shared = out_cnt_shared, j.out_cnt_notshared = out_cnt_notshared;
  return run_on_devices(j, num_devices, devices);
}

int colate_bootstrap_em_batch_groups_sharded(int num_devices, const int* devices, int G, int B, int E, int A,
                                             const double* age_grid, const int* group_nb, const double* group_age,
                                             const double* weights, const double* sh_block, const double* ns_block,
                                             const double* sh_emp_block, const double* ns_emp_block,
                                             const double* epochs, const double* init_rates, int max_iter,
                                             int min_iter, double rel_tol, double rate_floor, double* out_rates,
                                             int* out_iters, double* out_loglik, int* out_flags,
                                             double* out_cnt_shared, double* out_cnt_notshared) {
  if (G < 0 || B < 1) return fail(COLATE_EINVAL, "bad sizes G=%d B=%d", G, B);
  if ((long long)G * B > 0x7fffffffLL) return fail(COLATE_ELIMIT, "G x B = %lld rows", (long long)G * B);
  EmJob j = groups_job(G, B, 0, G, E, A, age_grid, group_nb, group_age, weights, sh_block, ns_block, sh_emp_block,
                       ns_emp_block, epochs, init_rates, max_iter, min_iter, rel_tol, rate_floor, out_rates, out_iters,
                       out_loglik, out_flags);
  j.out_cnt_shared = out_cnt_shared, j.out_cnt_notshared = out_cnt_notshared;
  return run_on_devices(j, num_devices, devices);
}

int colate_release_workspace(void) {
  thread_workspace().release();
  return COLATE_OK;
}

int colate_bootstrap_counts_device(int B, int nb, int A, const double* age_grid, double age, const double* weights,
                                   const double* sh_block, const double* ns_block, const double* sh_emp_block,
                                   const double* ns_emp_block, double* cnt_shared, double* cnt_notshared, int* status,
                                   void* hip_stream) {
  if (B < 0 || nb < 1 || A < 2 || A > COLATE_EM_MAX_A) return fail(COLATE_EINVAL, "bad sizes B=%d nb=%d A=%d", B, nb, A);
  if (!age_grid || !weights || !sh_block || !ns_block || !sh_emp_block || !ns_emp_block || !cnt_shared ||
      !cnt_notshared)
    return fail(COLATE_EINVAL, "NULL pointer argument");
  if (B == 0) return COLATE_OK;
  std::unique_ptr<void, hipError_t (*)(void*)> scratch(nullptr, hipFree);
  if (!status) {  // the kernel always reports; give it somewhere to write
    void* p = nullptr;
    HIP_TRY(hipMalloc(&p, sizeof(int)));
    scratch.reset(p);
    HIP_TRY(hipMemsetAsync(p, 0, sizeof(int), static_cast<hipStream_t>(hip_stream)));
  }
  hipError_t e = colate_bootstrap_launch(B, nb, A, age_grid, age, weights, sh_block, ns_block, sh_emp_block,
                                         ns_emp_block, cnt_shared, cnt_notshared,
                                         status ? status : static_cast<int*>(scratch.get()),
                                         static_cast<hipStream_t>(hip_stream));
  if (e != hipSuccess) return hip_fail(e, "bootstrap kernel launch");
  if (!status) HIP_TRY(hipStreamSynchronize(static_cast<hipStream_t>(hip_stream)));  // scratch dies with this call
  return COLATE_OK;
}

int colate_bootstrap_em_batch(int B, int nb, int E, int A, const double* age_grid, double age, const double* weights,
                              const double* sh_block, const double* ns_block, const double* sh_emp_block,
                              const double* ns_emp_block, const double* epochs, const double* init_rates, int max_iter,
                              int min_iter, double rel_tol, double rate_floor, double* out_rates, int* out_iters,
                              double* out_loglik, int* out_flags, double* out_cnt_shared, double* out_cnt_notshared) {
  EmJob j = genome_job(B, nb, E, A, age_grid, age, weights, sh_block, ns_block, sh_emp_block, ns_emp_block, epochs,
                       init_rates, max_iter, min_iter, rel_tol, rate_floor, out_rates, out_iters, out_loglik, out_flags);
  j.out_cnt_shared = out_cnt_shared, j.out_cnt_notshared = out_cnt_notshared;
  return run_here(j, "colate_bootstrap_em_batch: H2D + bootstrap kernel + EM kernel + D2H");
}

int colate_bootstrap_counts_groups_device(int G, int B, int group_first, int row_lo, int row_hi, int A,
                                          const double* age_grid, const int* group_nb,
                                          const long long* group_block_off, const long long* group_weight_off,
                                          const double* group_age, const double* weights, const double* sh_block,
                                          const double* ns_block, const double* sh_emp_block,
                                          const double* ns_emp_block, double* cnt_shared, double* cnt_notshared,
                                          int* status, void* hip_stream) {
  if (G < 1 || B < 1 || A < 2 || A > COLATE_EM_MAX_A || group_first < 0 || row_lo < 0 || row_hi < row_lo)
    return fail(COLATE_EINVAL, "bad sizes G=%d B=%d A=%d rows [%d, %d)", G, B, A, row_lo, row_hi);
  if (row_hi > row_lo && (row_lo / B < group_first || (row_hi - 1) / B >= group_first + G))
    return fail(COLATE_EINVAL, "rows [%d, %d) lie outside groups [%d, %d)", row_lo, row_hi, group_first, group_first + G);
  if (!age_grid || !group_nb || !group_block_off || !group_weight_off || !group_age || !weights || !sh_block ||
      !ns_block || !sh_emp_block || !ns_emp_block || !cnt_shared || !cnt_notshared || !status)
    return fail(COLATE_EINVAL, "NULL pointer argument");
  if (row_hi == row_lo) return COLATE_OK;
  mark_device_touched();
  hipError_t e = colate_bootstrap_groups_launch(B, row_lo, row_hi - row_lo, group_first, A, age_grid, group_nb,
                                                group_block_off, group_weight_off, group_age, weights, sh_block,
                                                ns_block, sh_emp_block, ns_emp_block, cnt_shared, cnt_notshared,
                                                status, static_cast<hipStream_t>(hip_stream));
  if (e != hipSuccess) return hip_fail(e, "bootstrap kernel launch");
  return COLATE_OK;
}

int colate_bootstrap_em_batch_groups(int G, int B, int E, int A, const double* age_grid, const int* group_nb,
                                     const double* group_age, const double* weights, const double* sh_block,
                                     const double* ns_block, const double* sh_emp_block,
                                     const double* ns_emp_block, const double* epochs, const double* init_rates,
                                     int max_iter, int min_iter, double rel_tol, double rate_floor,
                                     double* out_rates, int* out_iters, double* out_loglik, int* out_flags,
                                     double* out_cnt_shared, double* out_cnt_notshared) {
  if (G < 0 || B < 1) return fail(COLATE_EINVAL, "bad sizes G=%d B=%d", G, B);
  if ((long long)G * B > 0x7fffffffLL) return fail(COLATE_ELIMIT, "G x B = %lld rows", (long long)G * B);
  EmJob j = groups_job(G, B, 0, G, E, A, age_grid, group_nb, group_age, weights, sh_block, ns_block, sh_emp_block,
                       ns_emp_block, epochs, init_rates, max_iter, min_iter, rel_tol, rate_floor, out_rates, out_iters,
                       out_loglik, out_flags);
  j.out_cnt_shared = out_cnt_shared, j.out_cnt_notshared = out_cnt_notshared;
  return run_here(j, "colate_bootstrap_em_batch_groups: H2D + bootstrap kernel + EM kernel + D2H");
}

int colate_em_estep(int B, int E, int A, const double* age_grid, const double* cnt_shared, const double* cnt_notshared,
                    const double* epochs, const double* rates, double* num_acc, double* den_acc, double* loglik,
                    int* flags) {
  if (int rc = check_sizes(B, E, A)) return rc;
  if (!age_grid || !cnt_shared || !cnt_notshared || !epochs || !rates || !num_acc || !den_acc ||
      !loglik || !flags)
    return fail(COLATE_EINVAL, "NULL pointer argument");
  if (int rc = check_grids(E, A, age_grid, epochs)) return rc;
  if (int rc = ensure_device()) return rc;
  if (B == 0) return COLATE_OK;
  const size_t nBA = (size_t)B * A, nBE = (size_t)B * E;
  Arena st(thread_workspace());
  const int i_grid = st.in(age_grid, A), i_sh = st.in(cnt_shared, nBA), i_ns = st.in(cnt_notshared, nBA);
  const int i_ep = st.in(epochs, E), i_rates = st.in(rates, nBE);
  const int o_num = st.out(num_acc, nBE), o_den = st.out(den_acc, nBE), o_ll = st.out(loglik, B), o_flags = st.out(flags, B);
  if (int rc = st.commit()) return rc;
  if (int rc = colate_em_estep_device(B, E, A, st.dev<double>(i_grid), st.dev<double>(i_sh), st.dev<double>(i_ns),
                                      st.dev<double>(i_ep), st.dev<double>(i_rates), st.dev<double>(o_num),
                                      st.dev<double>(o_den), st.dev<double>(o_ll), st.dev<int>(o_flags), st.stream()))
    return rc;
  return st.finish();
}

int colate_em_interval_calls(int R, int E, const int* kinds, const double* age_begin, const double* age_end,
                             const double* epochs, const double* rates, const double* weights, double* out_num,
                             double* out_den, double* out_logl, int* out_flags, double* out_num_acc, double* out_den_acc,
                             double* out_ll) {
  if (int rc = check_interval_calls(R, E, kinds, age_begin, age_end, epochs, rates, weights, out_num, out_den, out_logl,
                                    out_flags, out_num_acc, out_den_acc, out_ll))
    return rc;
  if (int rc = ensure_device()) return rc;
  const size_t nE = (size_t)E, nRE = (size_t)R * E, nacc = weights ? nE : 0;
  if (R == 0) {
    for (size_t e = 0; e < nacc; e++) out_num_acc[e] = 0.0, out_den_acc[e] = 0.0;
    if (weights) *out_ll = 0.0;
    return COLATE_OK;
  }
  ProfRange range("colate_em_interval_calls: H2D + interval E-step kernel + D2H");
  Arena st(thread_workspace());
  const int i_kind = st.in(kinds, R), i_a0 = st.in(age_begin, R), i_a1 = st.in(age_end, R);
  const int i_ep = st.in(epochs, nE), i_rates = st.in(rates, nE), i_w = st.in(weights, weights ? (size_t)R : 0);
  const int o_num = st.out(out_num, nRE), o_den = st.out(out_den, nRE), o_ll = st.out(out_logl, R), o_flags = st.out(out_flags, R);
  const int o_nacc = st.out(out_num_acc, nacc), o_dacc = st.out(out_den_acc, nacc), o_llsum = st.out(out_ll, weights ? 1 : 0);
  if (int rc = st.commit()) return rc;
  const hipError_t e = colate_em_interval_launch(R, E, st.dev<int>(i_kind), st.dev<double>(i_a0), st.dev<double>(i_a1),
                                                 st.dev<double>(i_ep), st.dev<double>(i_rates),
                                                 weights ? st.dev<double>(i_w) : nullptr, st.dev<double>(o_num),
                                                 st.dev<double>(o_den), st.dev<double>(o_ll), st.dev<int>(o_flags),
                                                 st.dev<double>(o_nacc), st.dev<double>(o_dacc), st.dev<double>(o_llsum),
                                                 st.stream());
  if (e != hipSuccess) return hip_fail(e, "interval E-step kernel launch");
  return st.finish();
}

int colate_em_interval_batch(int B, int R, int E, const int* kinds, const double* age_begin, const double* age_end,
                             const double* weights, const double* epochs, const double* init_rates, int max_iter,
                             int min_iter, double rel_tol, double rate_floor, double* out_rates, int* out_iters,
                             double* out_loglik, int* out_flags) {
  if (int rc = check_interval_batch(B, R, E, kinds, age_begin, age_end, weights, epochs, init_rates, max_iter, min_iter,
                                    rel_tol, rate_floor, out_rates, out_iters, out_loglik, out_flags))
    return rc;
  if (int rc = ensure_device()) return rc;
  ProfRange range("colate_em_interval_batch: H2D + interval EM kernel + D2H");
  const size_t nE = (size_t)E, nBE = (size_t)B * E;
  Arena st(thread_workspace());
  const int i_kind = st.in(kinds, R), i_a0 = st.in(age_begin, R), i_a1 = st.in(age_end, R);
  const int i_w = st.in(weights, (size_t)B * R), i_ep = st.in(epochs, nE), i_init = st.in(init_rates, nE);
  const int o_rates = st.out(out_rates, nBE), o_iters = st.out(out_iters, B), o_ll = st.out(out_loglik, B), o_flags = st.out(out_flags, B);
  if (int rc = st.commit()) return rc;
  const hipError_t e = colate_em_interval_fit_launch(B, R, E, st.dev<int>(i_kind), st.dev<double>(i_a0), st.dev<double>(i_a1),
                                                     st.dev<double>(i_w), st.dev<double>(i_ep), st.dev<double>(i_init),
                                                     max_iter, min_iter, rel_tol, rate_floor, st.dev<double>(o_rates),
                                                     st.dev<int>(o_iters), st.dev<double>(o_ll), st.dev<int>(o_flags),
                                                     st.stream());
  if (e != hipSuccess) return hip_fail(e, "interval EM kernel launch");
  return st.finish();
}

int colate_bootstrap_em_interval_batch(int B, int nb, int R, int E, const int* kinds, const double* age_begin,
                                       const double* age_end, const double* block_weights, const double* tables,
                                       const double* epochs, const double* init_rates, int max_iter, int min_iter,
                                       double rel_tol, double rate_floor, double* out_rates, int* out_iters,
                                       double* out_loglik, int* out_flags) {
  if (int rc = check_bootstrap_interval_batch(B, nb, R, E, kinds, age_begin, age_end, block_weights, tables, epochs, init_rates,
                                              max_iter, min_iter, rel_tol, rate_floor, out_rates, out_iters, out_loglik,
                                              out_flags))
    return rc;
  if (!colate_bootstrap_rows_fits(B, R)) return fail(COLATE_ELIMIT, "B=%d x R=%d above the grid of the bootstrap kernel", B, R);
  if (int rc = ensure_device()) return rc;
  ProfRange range("colate_bootstrap_em_interval_batch: H2D + row bootstrap kernel + interval EM kernel + D2H");
  const size_t nE = (size_t)E, nBE = (size_t)B * E;
  Arena st(thread_workspace());
  const int i_kind = st.in(kinds, R), i_a0 = st.in(age_begin, R), i_a1 = st.in(age_end, R);
  const int i_bw = st.in(block_weights, (size_t)B * nb), i_tab = st.in(tables, (size_t)nb * R);
  const int i_ep = st.in(epochs, nE), i_init = st.in(init_rates, nE);
  const int s_w = st.scratch<double>((size_t)B * R);  // W[B][R]: written by the first kernel, read by the second, never copied
  const int o_rates = st.out(out_rates, nBE), o_iters = st.out(out_iters, B), o_ll = st.out(out_loglik, B), o_flags = st.out(out_flags, B);
  if (int rc = st.commit()) return rc;
  hipError_t e = colate_bootstrap_rows_launch(B, nb, R, st.dev<double>(i_bw), st.dev<double>(i_tab), st.dev<double>(s_w), st.stream());
  if (e != hipSuccess) return hip_fail(e, "row bootstrap kernel launch");
  e = colate_em_interval_fit_launch(B, R, E, st.dev<int>(i_kind), st.dev<double>(i_a0), st.dev<double>(i_a1),
                                    st.dev<double>(s_w), st.dev<double>(i_ep), st.dev<double>(i_init), max_iter, min_iter,
                                    rel_tol, rate_floor, st.dev<double>(o_rates), st.dev<int>(o_iters), st.dev<double>(o_ll),
                                    st.dev<int>(o_flags), st.stream());
  if (e != hipSuccess) return hip_fail(e, "interval EM kernel launch");
  return st.finish();
}

int colate_em_interval_batch_waves(int E) { return colate_em_interval_fit_waves(E); }

int colate_interval_cells(long long n, const colate_interval_rec* recs, const int* block, int nb, int max_rows, int* kinds,
                          double* age_begin, double* age_end, double* tables, long long* dropped) {
  using namespace colate_ic;
  if (int rc = check_cells_args(n, recs, block, nb, max_rows, kinds, age_begin, age_end, tables, dropped)) return rc;
  float T[kBins];
  if (int rc = build_thresholds(T)) return rc;
  if (int rc = ensure_device()) return rc;
  ProfRange range("colate_interval_cells: H2D + bin kernel + cell-sum kernel + D2H");
  std::vector<long long> off((size_t)nb + 1);
  block_ranges(n, block, nb, off.data());
  std::vector<double> cells((size_t)nb * 2 * kCells);
  std::vector<unsigned long long> nd((size_t)nb);
  Arena st(thread_workspace());
  const int i_recs = st.in(recs, (size_t)n), i_off = st.in(off.data(), off.size()), i_T = st.in(T, (size_t)kBins);
  const int s_idx = st.scratch<int>((size_t)n);
  const int o_cells = st.out(cells.data(), cells.size()), o_nd = st.out(nd.data(), nd.size());
  if (int rc = st.commit()) return rc;
  const hipError_t e = colate_interval_cells_launch(n, st.dev<IntervalRec>(i_recs), st.dev<long long>(i_off), nb, st.dev<float>(i_T),
                                                    st.dev<int>(s_idx), st.dev<double>(o_cells),
                                                    st.dev<unsigned long long>(o_nd), st.stream());
  if (e != hipSuccess) return hip_fail(e, "interval cells kernel launch");
  if (int rc = st.finish()) return rc;
  const int R = compact_cells(nb, cells.data(), max_rows, kinds, age_begin, age_end, tables);
  if (R < 0) return R;
  unsigned long long total = 0;
  for (unsigned long long d : nd) total += d;
  *dropped = (long long)total;
  return R;
}

}  // extern "C"
