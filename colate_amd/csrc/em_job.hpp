// colate_amd/csrc/em_job.hpp -- what the host-pointer EM entry points share (colate_api.cpp, colate_comm.cpp): one
// description of a call (EmJob), one validator, one staging arena and one function that enqueues a range of rows.
// An entry point fills in the description, validates it and picks where the rows run: on this thread's workspace,
// sharded over a list of devices, or on a communicator's rank.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <vector>

#include "colate_amd.h"
#include "colate_internal.h"

namespace colate {

// COLATE_ENODEVICE where HIP reports that there is no (such) device, COLATE_EHIP otherwise
int hip_fail(hipError_t e, const char* what);
#define HIP_TRY(expr)                                          \
  do {                                                         \
    hipError_t e_ = (expr);                                    \
    if (e_ != hipSuccess) return ::colate::hip_fail(e_, #expr); \
  } while (0)

// One EM call over R rows.  Pointers to the caller's host arrays; nothing is owned.
struct EmJob {
  enum Source { kTables, kGenome, kGroups };    // where the counts of a row come from
  enum Layout { kShared, kPerRow, kPerGroup };  // epochs / init_rates: [E], [R][E], [group_count][E]
  int R = 0, E = 0, A = 0;
  const double* age_grid = nullptr;
  Source source = kTables;
  const double *cnt_shared = nullptr, *cnt_notshared = nullptr;  // kTables: [R][A]
  // kGenome: weights [R][nb] and four block tables [nb][A] (bootstrap_kernel).  kGroups: row r is replicate r % B of
  // group r / B; the arrays describe groups [group_first, group_first + group_count), weights ([B][nb[g]] per group)
  // and block tables concatenated (bootstrap_groups_kernel).
  int nb = 0;
  double age = 0;
  int B = 0, group_first = 0, group_count = 0;
  const int* group_nb = nullptr;
  const double* group_age = nullptr;
  const double* weights = nullptr;
  const double* block[4] = {nullptr, nullptr, nullptr, nullptr};  // sh, ns, sh_emp, ns_emp
  Layout layout = kShared;
  const double *epochs = nullptr, *init_rates = nullptr;
  int max_iter = 0, min_iter = 0;
  double rel_tol = 0, rate_floor = 0;
  double* out_rates = nullptr;  // [R][E]
  int* out_iters = nullptr;     // [R]
  double* out_loglik = nullptr;
  int* out_flags = nullptr;
  double *out_cnt_shared = nullptr, *out_cnt_notshared = nullptr;  // optional (not kTables): [R][A]
  double* ll_trace = nullptr;                                      // optional: [R][ll_trace_cap] (COLATE_LL_TRACE)
  int ll_trace_cap = 0;
};

// The three count sources as the entry points name them (the argument lists of include/colate_amd.h).
inline EmJob tables_job(EmJob::Layout layout, int R, int E, int A, const double* age_grid, const double* cnt_shared,
                        const double* cnt_notshared, const double* epochs, const double* init_rates, int max_iter,
                        int min_iter, double rel_tol, double rate_floor, double* out_rates, int* out_iters,
                        double* out_loglik, int* out_flags) {
  EmJob j;
  j.R = R, j.E = E, j.A = A, j.age_grid = age_grid, j.cnt_shared = cnt_shared, j.cnt_notshared = cnt_notshared;
  j.layout = layout, j.epochs = epochs, j.init_rates = init_rates;
  j.max_iter = max_iter, j.min_iter = min_iter, j.rel_tol = rel_tol, j.rate_floor = rate_floor;
  j.out_rates = out_rates, j.out_iters = out_iters, j.out_loglik = out_loglik, j.out_flags = out_flags;
  return j;
}
inline EmJob genome_job(int R, int nb, int E, int A, const double* age_grid, double age, const double* weights,
                        const double* sh_block, const double* ns_block, const double* sh_emp_block,
                        const double* ns_emp_block, const double* epochs, const double* init_rates, int max_iter,
                        int min_iter, double rel_tol, double rate_floor, double* out_rates, int* out_iters,
                        double* out_loglik, int* out_flags) {
  EmJob j = tables_job(EmJob::kShared, R, E, A, age_grid, nullptr, nullptr, epochs, init_rates, max_iter, min_iter,
                       rel_tol, rate_floor, out_rates, out_iters, out_loglik, out_flags);
  j.source = EmJob::kGenome, j.nb = nb, j.age = age, j.weights = weights;
  j.block[0] = sh_block, j.block[1] = ns_block, j.block[2] = sh_emp_block, j.block[3] = ns_emp_block;
  return j;
}
// (G groups x B replicates = G * B rows, which the caller has found to fit an int)
inline EmJob groups_job(int G, int B, int group_first, int group_count, int E, int A, const double* age_grid,
                        const int* group_nb, const double* group_age, const double* weights, const double* sh_block,
                        const double* ns_block, const double* sh_emp_block, const double* ns_emp_block,
                        const double* epochs, const double* init_rates, int max_iter, int min_iter, double rel_tol,
                        double rate_floor, double* out_rates, int* out_iters, double* out_loglik, int* out_flags) {
  EmJob j = genome_job(G * B, 0, E, A, age_grid, 0, weights, sh_block, ns_block, sh_emp_block, ns_emp_block, epochs,
                       init_rates, max_iter, min_iter, rel_tol, rate_floor, out_rates, out_iters, out_loglik, out_flags);
  j.source = EmJob::kGroups, j.layout = EmJob::kPerGroup;
  j.B = B, j.group_first = group_first, j.group_count = group_count, j.group_nb = group_nb, j.group_age = group_age;
  return j;
}

// The only argument checks of the host-pointer EM calls, before a device is asked for.  check_call: what every rank
// of a collective sees alike (sizes, compiled limits, max_iter, the arrays every caller brings); check_inputs: the
// count source, epochs and starting rates (NULLs, group_nb >= 1, check_grids per distinct epoch row).
int check_call(const EmJob& job);
int check_inputs(const EmJob& job);
inline int check(const EmJob& job) {
  if (int rc = check_call(job)) return rc;
  return check_inputs(job);
}

// Backing store of an Arena: one device buffer, one pinned host buffer, one stream, grown on demand and kept.  Owned
// by the calling thread's workspace, by a shard of a devices-list call, or by a communicator.
struct ArenaStore {
  int device = -1;
  char* d = nullptr;
  size_t dcap = 0;
  char* h = nullptr;
  size_t hcap = 0;
  hipStream_t stream = nullptr;
  int reserve(size_t dbytes, size_t hbytes);  // on the current device; a store that lived on another one starts over
  void release();                             // on the owning device; the caller's current device is restored
};
// the calling thread's workspace (colate_api.cpp): kept between calls, freed by colate_release_workspace or with the thread
ArenaStore& thread_workspace();

// One staged call on a store: declare what goes in, what stays on the device and what comes out, commit() (one H2D
// copy), launch on stream(), finish() (one D2H copy, one synchronise, scatter to the caller).
class Arena {
 public:
  explicit Arena(ArenaStore& store) : st_(&store) {}
  template <typename T>
  int in(const T* host, size_t n) {  // host is read by commit()
    return add(kIn, host, nullptr, n * sizeof(T));
  }
  template <typename T>
  int out(T* host, size_t n) {  // host may be NULL: the space exists on the device, nothing is returned
    return add(kOut, nullptr, host, n * sizeof(T));
  }
  template <typename T>
  int scratch(size_t n) {
    return add(kScratch, nullptr, nullptr, n * sizeof(T));
  }
  template <typename T>
  T* dev(int idx) const {
    return reinterpret_cast<T*>(st_->d + seg_[idx].doff);
  }
  hipStream_t stream() const { return st_->stream; }
  int commit();
  int finish();  // (nothing to do on an arena that was never committed)

 private:
  enum Kind { kIn = 0, kScratch = 1, kOut = 2 };
  struct Seg {
    Kind kind;
    const void* src;
    void* dst;
    size_t bytes, koff = 0, doff = 0;
  };
  int add(Kind k, const void* src, void* dst, size_t bytes) {
    seg_.push_back(Seg{k, src, dst, bytes});
    return (int)seg_.size() - 1;
  }
  std::vector<Seg> seg_;
  ArenaStore* st_;
  bool committed_ = false;
  size_t in_bytes_ = 0, out_bytes_ = 0, out_base_ = 0;
};

// where the four results of a range of rows go on the device; all NULL = `out` segments of the arena, which finish()
// returns to the job's rows
struct RowOut {
  double* rates = nullptr;
  double* loglik = nullptr;
  int* iters = nullptr;
  int* flags = nullptr;
};

// Stages what rows [lo, hi) of the job need (their slice of the tables / weights, the groups they belong to, epochs
// and starting rates per row where the layout is per group), commits, and enqueues the bootstrap kernel (unless the
// source is tables) and the EM kernel on the arena's stream.  *status receives the bootstrap kernel's status word
// with finish(); finish_rows() is finish() plus that word's error.
int enqueue_rows(const EmJob& job, int lo, int hi, Arena& arena, int* status, RowOut out = RowOut());
int finish_rows(Arena& arena, const int& status);

}  // namespace colate
