// colate_amd/csrc/colate_comm.cpp -- the one-process-per-GPU form of the replicate sharding, in C++:
// every rank runs its contiguous range of bootstrap replicates on its own GPU and ONE ncclAllGather (RCCL over
// xGMI) hands every rank all results.  There is no counterpart in the reference (its mut() loops over the
// replicates sequentially, include/coal/coal.cpp:3675-3846); SURVEY.md section 8(e) defines this row.
//
// RCCL is bound lazily with dlopen: a process that never creates a communicator never loads it, and inside a
// process that already carries an RCCL (PyTorch ships its own librccl.so.1) the same copy is used instead of a
// second one with the same SONAME.
#include <dlfcn.h>
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "colate_amd.h"
#include "colate_internal.h"
#include "em_job.hpp"

static_assert(COLATE_COMM_ID_BYTES == NCCL_UNIQUE_ID_BYTES, "unique id size");

namespace {

using namespace colate;

struct Rccl {
  void* handle = nullptr;
  ncclResult_t (*GetUniqueId)(ncclUniqueId*) = nullptr;
  ncclResult_t (*CommInitRank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
  ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
  ncclResult_t (*AllGather)(const void*, void*, size_t, ncclDataType_t, ncclComm_t, hipStream_t) = nullptr;
  const char* (*GetErrorString)(ncclResult_t) = nullptr;
  const char* error = nullptr;
};

Rccl& rccl() {
  static Rccl r;
  static std::once_flag once;
  std::call_once(once, [] {
    for (const char* name : {"librccl.so.1", "/opt/rocm/lib/librccl.so.1", "librccl.so"}) {
      r.handle = dlopen(name, RTLD_NOW | RTLD_LOCAL);
      if (r.handle) break;
    }
    if (!r.handle) {
      r.error = "librccl.so.1 could not be loaded";
      return;
    }
    auto sym = [&](const char* n) {
      void* p = dlsym(r.handle, n);
      if (!p) r.error = "RCCL symbol missing";
      return p;
    };
    r.GetUniqueId = reinterpret_cast<decltype(r.GetUniqueId)>(sym("ncclGetUniqueId"));
    r.CommInitRank = reinterpret_cast<decltype(r.CommInitRank)>(sym("ncclCommInitRank"));
    r.CommDestroy = reinterpret_cast<decltype(r.CommDestroy)>(sym("ncclCommDestroy"));
    r.AllGather = reinterpret_cast<decltype(r.AllGather)>(sym("ncclAllGather"));
    r.GetErrorString = reinterpret_cast<decltype(r.GetErrorString)>(sym("ncclGetErrorString"));
  });
  return r;
}

int rccl_ready() {
  Rccl& r = rccl();
  if (r.error) return fail(COLATE_EHIP, "RCCL unavailable: %s", r.error);
  return COLATE_OK;
}

#define NCCL_TRY(expr)                                                                         \
  do {                                                                                         \
    ncclResult_t r_ = (expr);                                                                  \
    if (r_ != ncclSuccess) return fail(COLATE_EHIP, "%s: %s", #expr, rccl().GetErrorString(r_)); \
  } while (0)

struct Comm {
  ncclComm_t nccl = nullptr;
  int nranks = 1, rank = 0, device = 0;
  ArenaStore store;  // the rank's inputs and scratch (em_job.hpp); its stream is the communicator's
  char* d_send = nullptr;
  char* d_recv = nullptr;
  size_t cap = 0;  // bytes per rank the two buffers are sized for
  char* h_recv = nullptr;
  size_t hcap = 0;
};

// bytes of one rank's packed results: rates[n_max][E] f64 | loglik[n_max] f64 | iters[n_max] i32 | flags[n_max] i32 |
// this rank's return code (i32, padded to 8): a rank whose local work failed still takes part in the collective --
// otherwise the others would wait for it forever -- and every rank learns of the failure from the gathered codes
size_t payload_bytes(int n_max, int E) { return (size_t)n_max * ((size_t)E * 8 + 8 + 4 + 4); }
size_t packed_bytes(int n_max, int E) { return ((payload_bytes(n_max, E) + 7) & ~size_t(7)) + 8; }

// the two device buffers of the collective; without them this rank cannot take part in it
int reserve_device(Comm* c, size_t per_rank) {
  if (per_rank > c->cap) {
    if (c->d_send) (void)hipFree(c->d_send);
    if (c->d_recv) (void)hipFree(c->d_recv);
    c->d_send = c->d_recv = nullptr, c->cap = 0;
    HIP_TRY(hipMalloc(reinterpret_cast<void**>(&c->d_send), per_rank));
    HIP_TRY(hipMalloc(reinterpret_cast<void**>(&c->d_recv), per_rank * c->nranks));
    c->cap = per_rank;
  }
  return COLATE_OK;
}
// the pinned landing buffer of the gathered results
int reserve_host(Comm* c, size_t per_rank) {
  if (per_rank * c->nranks > c->hcap) {
    if (c->h_recv) (void)hipHostFree(c->h_recv);
    c->h_recv = nullptr, c->hcap = 0;
    HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&c->h_recv), per_rank * c->nranks, hipHostMallocDefault));
    c->hcap = per_rank * c->nranks;
  }
  return COLATE_OK;
}

// Run this rank's rows [lo, hi) of the job on the communicator's arena with the four outputs placed directly in the send
// buffer, all-gather, and scatter every rank's part into the job's output arrays.  `early`: what this rank already
// found wrong with its own inputs (message in colate_last_error()).
int run_and_gather(Comm* c, const EmJob& job, int early = COLATE_OK) {
  const std::string early_msg = early ? colate_last_error() : "";
  if (int rc = ensure_device()) return rc;
  if (job.R == 0) return COLATE_OK;
  // Everything that can fail on THIS rank before the collective is turned into `local_rc`, and the rank still joins the
  // all-gather with its code in the trailing slot: a rank that returned early would leave the others waiting in
  // ncclAllGather forever.  The one exception is a rank that cannot even get its two device buffers (or its device): it
  // has nothing to join with and returns -- `Colate --ranks` (run_ranked) then ends the remaining ranks after a grace
  // period; a host that drives the ranks itself needs the same watchdog.
  HIP_TRY(hipSetDevice(c->device));
  const int B = job.R, E = job.E;
  const hipStream_t stream = c->store.stream;
  const int n_max = (B + c->nranks - 1) / c->nranks;
  const size_t per_rank = packed_bytes(n_max, E);
  if (int rc = reserve_device(c, per_rank)) return rc;
  int local_rc = reserve_host(c, per_rank);
  int lo = 0, hi = 0;
  colate_shard_bounds(B, c->nranks, c->rank, &lo, &hi);
  auto carve = [&](char* base) {
    RowOut o;
    o.rates = reinterpret_cast<double*>(base);
    o.loglik = o.rates + (size_t)n_max * E;
    o.iters = reinterpret_cast<int*>(o.loglik + n_max);
    o.flags = o.iters + n_max;
    return o;
  };
  if (!local_rc) {  // rows of a short shard beyond its n stay zero
    const hipError_t e = hipMemsetAsync(c->d_send, 0, per_rank, stream);
    if (e != hipSuccess) local_rc = hip_fail(e, "hipMemsetAsync");
  }
#ifdef COLATE_TEST_HOOKS  // (only in lib/testhooks/libcolate_amd.so: failure injection for the tests of exactly this path)
  if (const char* inj = getenv("COLATE_TEST_FAIL_RANK")) {
    if (atoi(inj) == c->rank) local_rc = fail(COLATE_EHIP, "injected failure on rank %d (COLATE_TEST_FAIL_RANK)", c->rank);
  }
#endif
  Arena arena(c->store);
  int status = 0;  // the bootstrap kernel's status word, read back after the collective
  if (!local_rc && hi > lo) {
    ProfRange range("colate shard: bootstrap + EM on this rank's replicates");
    local_rc = early ? fail(early, "%s", early_msg.c_str()) : enqueue_rows(job, lo, hi, arena, &status, carve(c->d_send));
  }
  std::string local_msg = local_rc ? colate_last_error() : "";
  if (local_rc) (void)hipMemcpyAsync(c->d_send + per_rank - 8, &local_rc, sizeof(int), hipMemcpyHostToDevice, stream);
  // the ONE collective of the path: per_rank bytes from every rank to every rank
  ProfRange gather_range("colate all-gather of the packed results (RCCL)");
  NCCL_TRY(rccl().AllGather(c->d_send, c->d_recv, per_rank, ncclChar, c->nccl, stream));
  if (c->h_recv && c->hcap >= per_rank * c->nranks)
    HIP_TRY(hipMemcpyAsync(c->h_recv, c->d_recv, per_rank * c->nranks, hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipStreamSynchronize(stream));
  if (local_rc) return fail(local_rc, "%s", local_msg.c_str());  // this rank's own message
  for (int r = 0; r < c->nranks; r++) {
    int code = 0;
    std::memcpy(&code, c->h_recv + (size_t)(r + 1) * per_rank - 8, sizeof(int));
    if (code) return fail(code, "rank %d of %d failed (code %d); see its own error output", r, c->nranks, code);
  }
  for (int r = 0; r < c->nranks; r++) {
    int rlo = 0, rhi = 0;
    colate_shard_bounds(B, c->nranks, r, &rlo, &rhi);
    const size_t n = (size_t)(rhi - rlo);
    const RowOut h = carve(c->h_recv + (size_t)r * per_rank);
    std::memcpy(job.out_rates + (size_t)rlo * E, h.rates, n * E * sizeof(double));
    std::memcpy(job.out_loglik + rlo, h.loglik, n * sizeof(double));
    std::memcpy(job.out_iters + rlo, h.iters, n * sizeof(int));
    std::memcpy(job.out_flags + rlo, h.flags, n * sizeof(int));
  }
  return finish_rows(arena, status);
}

}  // namespace

extern "C" {

int colate_shard_bounds(int B, int nranks, int rank, int* lo, int* hi) {
  if (B < 0 || nranks < 1 || rank < 0 || rank >= nranks || !lo || !hi) return fail(COLATE_EINVAL, "bad shard arguments");
  const int base = B / nranks, rem = B % nranks;
  *lo = rank * base + (rank < rem ? rank : rem);
  *hi = *lo + base + (rank < rem ? 1 : 0);
  return COLATE_OK;
}

int colate_comm_unique_id(void* id) {
  if (!id) return fail(COLATE_EINVAL, "NULL pointer argument");
  colate::mark_device_touched();
  if (int rc = rccl_ready()) return rc;
  ncclUniqueId u;
  NCCL_TRY(rccl().GetUniqueId(&u));
  std::memcpy(id, &u, sizeof(u));
  return COLATE_OK;
}

int colate_comm_create(const void* id, int nranks, int rank, void** comm) {
  if (!id || !comm || nranks < 1 || rank < 0 || rank >= nranks) return fail(COLATE_EINVAL, "bad communicator arguments");
  if (int rc = rccl_ready()) return rc;
  colate::mark_device_touched();
  Comm* c = new Comm;
  c->nranks = nranks, c->rank = rank;
  ncclUniqueId u;
  std::memcpy(&u, id, sizeof(u));
  hipError_t e = hipGetDevice(&c->device);
  if (e == hipSuccess) e = hipStreamCreateWithFlags(&c->store.stream, hipStreamNonBlocking);
  c->store.device = c->device;
  if (e != hipSuccess) {
    delete c;
    return fail(COLATE_ENODEVICE, "colate_comm_create: %s", hipGetErrorString(e));
  }
  ncclResult_t r = rccl().CommInitRank(&c->nccl, nranks, u, rank);
  if (r != ncclSuccess) {
    c->store.release();
    delete c;
    return fail(COLATE_EHIP, "ncclCommInitRank: %s", rccl().GetErrorString(r));
  }
  *comm = c;
  return COLATE_OK;
}

int colate_comm_destroy(void* comm) {
  Comm* c = static_cast<Comm*>(comm);
  if (!c) return COLATE_OK;
  (void)hipSetDevice(c->device);
  if (c->nccl) (void)rccl().CommDestroy(c->nccl);
  c->store.release();
  if (c->d_send) (void)hipFree(c->d_send);
  if (c->d_recv) (void)hipFree(c->d_recv);
  if (c->h_recv) (void)hipHostFree(c->h_recv);
  delete c;
  return COLATE_OK;
}

int colate_em_batch_allgather(void* comm, int B, int E, int A, const double* age_grid, const double* cnt_shared,
                              const double* cnt_notshared, const double* epochs, const double* init_rates,
                              int max_iter, int min_iter, double rel_tol, double rate_floor, double* out_rates,
                              int* out_iters, double* out_loglik, int* out_flags) {
  const EmJob j = tables_job(EmJob::kShared, B, E, A, age_grid, cnt_shared, cnt_notshared, epochs, init_rates, max_iter,
                             min_iter, rel_tol, rate_floor, out_rates, out_iters, out_loglik, out_flags);
  // (the same inputs on every rank: bad ones are refused by all of them alike, none enters the collective)
  if (int rc = check(j)) return rc;
  if (!comm) return fail(COLATE_EINVAL, "NULL communicator");
  return run_and_gather(static_cast<Comm*>(comm), j);
}

int colate_bootstrap_em_batch_allgather(void* comm, int B, int nb, int E, int A, const double* age_grid, double age,
                                        const double* weights, const double* sh_block, const double* ns_block,
                                        const double* sh_emp_block, const double* ns_emp_block, const double* epochs,
                                        const double* init_rates, int max_iter, int min_iter, double rel_tol,
                                        double rate_floor, double* out_rates, int* out_iters, double* out_loglik,
                                        int* out_flags) {
  const EmJob j = genome_job(B, nb, E, A, age_grid, age, weights, sh_block, ns_block, sh_emp_block, ns_emp_block, epochs,
                             init_rates, max_iter, min_iter, rel_tol, rate_floor, out_rates, out_iters, out_loglik,
                             out_flags);
  if (int rc = check(j)) return rc;
  if (!comm) return fail(COLATE_EINVAL, "NULL communicator");
  return run_and_gather(static_cast<Comm*>(comm), j);
}

int colate_bootstrap_em_batch_groups_allgather(void* comm, int G, int B, int group_first, int group_count, int E, int A,
                                               const double* age_grid, const int* group_nb, const double* group_age,
                                               const double* weights, const double* sh_block, const double* ns_block,
                                               const double* sh_emp_block, const double* ns_emp_block,
                                               const double* epochs, const double* init_rates, int max_iter,
                                               int min_iter, double rel_tol, double rate_floor, double* out_rates,
                                               int* out_iters, double* out_loglik, int* out_flags) {
  Comm* c = static_cast<Comm*>(comm);
  if (G < 0 || B < 1 || (long long)G * B > 0x7fffffffLL)
    return fail(COLATE_EINVAL, "bad sizes G=%d B=%d E=%d A=%d", G, B, E, A);
  const EmJob j = groups_job(G, B, group_first, group_count, E, A, age_grid, group_nb, group_age, weights, sh_block,
                             ns_block, sh_emp_block, ns_emp_block, epochs, init_rates, max_iter, min_iter, rel_tol,
                             rate_floor, out_rates, out_iters, out_loglik, out_flags);
  if (int rc = check_call(j)) return rc;  // (what every rank is given alike)
  if (!c) return fail(COLATE_EINVAL, "NULL communicator");
  int lo = 0, hi = 0;
  colate_shard_bounds(j.R, c->nranks, c->rank, &lo, &hi);
  // A rank with rows must bring exactly the groups they belong to.  A mismatch is this rank's own error and is found on
  // its inputs alone, but the other ranks may be fine: it joins the collective with its code (run_and_gather) instead of
  // leaving them waiting.
  int early = COLATE_OK;
  if (hi > lo) {
    if (group_first != lo / B || group_count != (hi - 1) / B - lo / B + 1)
      early = fail(COLATE_EINVAL, "rank %d computes rows [%d, %d) = groups [%d, %d], but was given groups [%d, %d)", c->rank, lo, hi,
                   lo / B, (hi - 1) / B, group_first, group_first + group_count);
    else
      early = check_inputs(j);
  }
  return run_and_gather(c, j, early);
}

}  // extern "C"
