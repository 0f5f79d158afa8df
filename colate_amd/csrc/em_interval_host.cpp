// colate_amd/csrc/em_interval_host.cpp -- the host side of the interval-dated E-step calls and of the EM fit over
// them: the argument checks of colate_em_interval_calls[_host], colate_em_interval_batch[_host] and
// colate_bootstrap_em_interval_batch[_host], the two host twins of em_interval_kernel.hip and
// em_interval_fit_kernel.hip (em_interval.hpp / em_interval_fit.hpp with <cmath> and with em_math.hpp) and the host
// twin of bootstrap_rows_kernel (the block bootstrap in front of the fit).  Plain C++: no device pass sees the <cmath>
// instantiation.
#include <cstring>
#include <vector>

#include "colate_amd.h"
#include "colate_internal.h"
#include "em_interval.hpp"
#include "em_interval_fit.hpp"

namespace colate {

int check_interval_calls(int R, int E, const int* kinds, const double* age_begin, const double* age_end,
                         const double* epochs, const double* rates, const double* weights, const double* out_num,
                         const double* out_den, const double* out_logl, const int* out_flags, const double* out_num_acc,
                         const double* out_den_acc, const double* out_ll) {
  if (R < 0 || E < 1) return fail(COLATE_EINVAL, "bad sizes R=%d E=%d", R, E);
  if (E > 1024) return fail(COLATE_ELIMIT, "E=%d above the compiled limit (1024)", E);
  if (!kinds || !age_begin || !age_end || !epochs || !rates || !out_num || !out_den || !out_logl || !out_flags)
    return fail(COLATE_EINVAL, "NULL pointer argument");
  if (weights && (!out_num_acc || !out_den_acc || !out_ll))
    return fail(COLATE_EINVAL, "weights given without out_num_acc / out_den_acc / out_ll");
  for (int e = 1; e < E; e++)
    if (!(epochs[e] >= epochs[e - 1])) return fail(COLATE_EINVAL, "epochs must be non-decreasing (index %d)", e);
  if (!(epochs[0] >= 0.0)) return fail(COLATE_EINVAL, "epochs[0] must not be negative");
  for (int r = 0; r < R; r++) {
    const double a0 = age_begin[r], a1 = age_end[r];
    if (kinds[r] != 0 && kinds[r] != 1) return fail(COLATE_EINVAL, "call %d: kind %d is neither 0 (shared) nor 1 (not shared)", r, kinds[r]);
    if (!(a0 >= 0.0) || !(a1 >= 0.0)) return fail(COLATE_EINVAL, "call %d: negative age (%g, %g)", r, a0, a1);
    if (!(a0 <= a1)) return fail(COLATE_EINVAL, "call %d: age_begin %g > age_end %g", r, a0, a1);
    if (!(a1 <= 0x1.fffffffffffffp+1023)) return fail(COLATE_EINVAL, "call %d: infinite age", r);
    if (!(epochs[0] <= a0)) return fail(COLATE_EINVAL, "call %d: age_begin %g lies before epochs[0]", r, a0);
  }
  return COLATE_OK;
}

// what check_interval_batch and check_bootstrap_interval_batch share: everything but the weights themselves
// (`weights_given`: the caller's weight arrays are not NULL)
static int check_interval_fit(int B, int R, int E, const int* kinds, const double* age_begin, const double* age_end,
                              bool weights_given, const double* epochs, const double* init_rates, int max_iter,
                              int min_iter, double rel_tol, double rate_floor, const double* out_rates,
                              const int* out_iters, const double* out_loglik, const int* out_flags) {
  const double huge = 0x1.fffffffffffffp+1023;
  if (B < 1 || R < 1) return fail(COLATE_EINVAL, "bad sizes B=%d R=%d (at least one replicate and one row)", B, R);
  if (!weights_given || !out_rates || !out_iters || !out_loglik || !out_flags) return fail(COLATE_EINVAL, "NULL pointer argument");
  // (rows, grid and E: the checks of the calls; init_rates stands in for the rates, the outputs are those above)
  if (int rc = check_interval_calls(R, E, kinds, age_begin, age_end, epochs, init_rates, nullptr, out_rates, out_rates,
                                    out_loglik, out_flags, nullptr, nullptr, nullptr))
    return rc;
  if (min_iter < 0) return fail(COLATE_EINVAL, "min_iter %d is negative", min_iter);
  if (max_iter < 1) return fail(COLATE_EINVAL, "max_iter %d: at least one iteration", max_iter);
  if (!(rel_tol > 0.0) || !(rel_tol <= huge)) return fail(COLATE_EINVAL, "rel_tol %g must be positive and finite", rel_tol);
  if (!(rate_floor >= 0.0)) return fail(COLATE_EINVAL, "rate_floor %g is negative", rate_floor);
  for (int e = 0; e < E; e++)
    if (!(init_rates[e] >= 0.0) || !(init_rates[e] <= huge))
      return fail(COLATE_EINVAL, "init_rates[%d] = %g must be finite and not negative", e, init_rates[e]);
  return COLATE_OK;
}

int check_interval_batch(int B, int R, int E, const int* kinds, const double* age_begin, const double* age_end,
                         const double* weights, const double* epochs, const double* init_rates, int max_iter, int min_iter,
                         double rel_tol, double rate_floor, const double* out_rates, const int* out_iters,
                         const double* out_loglik, const int* out_flags) {
  const double huge = 0x1.fffffffffffffp+1023;
  if (int rc = check_interval_fit(B, R, E, kinds, age_begin, age_end, weights != nullptr, epochs, init_rates, max_iter,
                                  min_iter, rel_tol, rate_floor, out_rates, out_iters, out_loglik, out_flags))
    return rc;
  for (size_t i = 0; i < (size_t)B * R; i++)
    if (!(weights[i] >= 0.0) || !(weights[i] <= huge))
      return fail(COLATE_EINVAL, "weight %g of replicate %zu, row %zu must be finite and not negative", weights[i], i / R, i % R);
  return COLATE_OK;
}

// W[b][r] = sum_k block_weights[b][k] * tables[k][r]: from 0.0, k ascending, every product rounded, then added (this file
// is compiled with -ffp-contract=off) -- per element the sum of bootstrap_rows_kernel (bootstrap_kernel.hip)
static void bootstrap_rows(int B, int nb, int R, const double* block_weights, const double* tables, double* W) {
  for (int b = 0; b < B; b++) {
    double* w = W + (size_t)b * R;
    for (int r = 0; r < R; r++) w[r] = 0.0;
    for (int k = 0; k < nb; k++) {
      const double wk = block_weights[(size_t)b * nb + k];
      const double* t = tables + (size_t)k * R;
      for (int r = 0; r < R; r++) w[r] += wk * t[r];
    }
  }
}

static int check_bootstrap_rows(int B, int nb, int R, const double* block_weights, const double* tables) {
  const double huge = 0x1.fffffffffffffp+1023;
  if (B < 1 || nb < 1 || R < 1)
    return fail(COLATE_EINVAL, "bad sizes B=%d nb=%d R=%d (at least one replicate, one genome block and one row)", B, nb, R);
  if (!block_weights || !tables) return fail(COLATE_EINVAL, "NULL pointer argument");
  for (size_t i = 0; i < (size_t)B * nb; i++)
    if (!(block_weights[i] >= 0.0) || !(block_weights[i] <= huge))
      return fail(COLATE_EINVAL, "block weight %g of replicate %zu, block %zu must be finite and not negative", block_weights[i],
                  i / nb, i % nb);
  for (size_t i = 0; i < (size_t)nb * R; i++)
    if (!(tables[i] >= 0.0) || !(tables[i] <= huge))
      return fail(COLATE_EINVAL, "table entry %g of block %zu, row %zu must be finite and not negative", tables[i], i / R, i % R);
  return COLATE_OK;
}

static int check_rows_finite(int B, int R, const double* W) {
  for (size_t i = 0; i < (size_t)B * R; i++)
    if (!(W[i] <= 0x1.fffffffffffffp+1023))
      return fail(COLATE_EINVAL, "the weighted block sum of replicate %zu, row %zu overflows", i / R, i % R);
  return COLATE_OK;
}

int check_bootstrap_interval_batch(int B, int nb, int R, int E, const int* kinds, const double* age_begin,
                                   const double* age_end, const double* block_weights, const double* tables,
                                   const double* epochs, const double* init_rates, int max_iter, int min_iter,
                                   double rel_tol, double rate_floor, const double* out_rates, const int* out_iters,
                                   const double* out_loglik, const int* out_flags) {
  if (nb < 1) return fail(COLATE_EINVAL, "bad size nb=%d (at least one genome block)", nb);
  if (int rc = check_interval_fit(B, R, E, kinds, age_begin, age_end, block_weights && tables, epochs, init_rates, max_iter,
                                  min_iter, rel_tol, rate_floor, out_rates, out_iters, out_loglik, out_flags))
    return rc;
  if (int rc = check_bootstrap_rows(B, nb, R, block_weights, tables)) return rc;
  // No entry of W is infinite.  All terms are >= 0, so a sum of nb products is at most nb * wmax * tmax * (1 + nb * 2^-52):
  // where that is below DBL_MAX / 2 nothing overflows; only otherwise are the sums formed here as well.
  double wmax = 0.0, tmax = 0.0;
  for (size_t i = 0; i < (size_t)B * nb; i++) wmax = block_weights[i] > wmax ? block_weights[i] : wmax;
  for (size_t i = 0; i < (size_t)nb * R; i++) tmax = tables[i] > tmax ? tables[i] : tmax;
  if (wmax * tmax * (double)nb <= 0x1.fffffffffffffp+1022) return COLATE_OK;
  std::vector<double> W((size_t)B * R);
  bootstrap_rows(B, nb, R, block_weights, tables, W.data());
  return check_rows_finite(B, R, W.data());
}

namespace {
// coal.cpp:3675-3827 with rows for age bins, one replicate after the other (em_interval_fit_kernel.hip: one workgroup each)
template <class M>
void run_fit(const M& m, int B, int R, int E, const int* kinds, const double* age_begin, const double* age_end,
             const double* weights, const double* epochs, const double* init_rates, int max_iter, int min_iter,
             double rel_tol, double rate_floor, double* out_rates, int* out_iters, double* out_loglik, int* out_flags) {
  std::vector<double> A(E), Bv(E), work(E), num(E), den(E), num_acc(E), den_acc(E);
  for (int b = 0; b < B; b++) {
    double* rates = out_rates + (size_t)b * E;
    const double* w_b = weights + (size_t)b * R;
    for (int e = 0; e < E; e++) rates[e] = init_rates[e];
    double ll = em_interval::log_zero(), prev_ll = ll;
    int flags = 0, iter = 0;
    for (; iter < max_iter; iter++) {
      em_interval::ab_prefix(E, epochs, rates, work.data());
      for (int e = 0; e < E; e++) em_interval::ab_at(m, E, epochs, rates, work.data(), e, A.data(), Bv.data());
      const em_interval::View v{E, epochs, rates, A.data(), Bv.data()};
      for (int e = 0; e < E; e++) num_acc[e] = 0.0, den_acc[e] = 0.0;
      prev_ll = ll;
      ll = 0.0;
      for (int r = 0; r < R; r++) {
        const double w = w_b[r];
        if (!(w > 0)) continue;  // (the reference visits bins with a count only)
        const double logl = em_interval::call(m, v, kinds[r], age_begin[r], age_end[r], num.data(), den.data(), work.data());
        ll += w * logl;
        for (int e = 0; e < E; e++) {
          flags |= em_interval::value_flags(num[e], den[e]);
          num_acc[e] += w * num[e];
          den_acc[e] += w * den[e];
        }
      }
      em_interval::mstep(E, num_acc.data(), den_acc.data(), rate_floor, rates);
      if (em_interval::stop_rule(ll, prev_ll, rel_tol, iter, min_iter)) break;
    }
    if (iter == max_iter) flags |= COLATE_FLAG_MAXITER;
    out_iters[b] = iter;
    out_loglik[b] = ll;
    out_flags[b] = flags;
  }
}

template <class M>
void run_calls(const M& m, int R, int E, const int* kinds, const double* age_begin, const double* age_end,
               const double* epochs, const double* rates, const double* weights, double* out_num, double* out_den,
               double* out_logl, int* out_flags, double* out_num_acc, double* out_den_acc, double* out_ll) {
  std::vector<double> A(E), B(E), work(E);
  em_interval::ab_prefix(E, epochs, rates, work.data());
  for (int e = 0; e < E; e++) em_interval::ab_at(m, E, epochs, rates, work.data(), e, A.data(), B.data());
  const em_interval::View v{E, epochs, rates, A.data(), B.data()};
  for (int r = 0; r < R; r++) {
    double *num = out_num + (size_t)r * E, *den = out_den + (size_t)r * E;
    out_logl[r] = em_interval::call(m, v, kinds[r], age_begin[r], age_end[r], num, den, work.data());
    int flags = 0;
    for (int e = 0; e < E; e++) flags |= em_interval::value_flags(num[e], den[e]);
    out_flags[r] = flags;
  }
  if (!weights) return;
  // coal.cpp:3704-3733 with weights for counts: rows in ascending order, rows without weight not visited
  double ll = 0.0;
  for (int e = 0; e < E; e++) out_num_acc[e] = 0.0, out_den_acc[e] = 0.0;
  for (int r = 0; r < R; r++) {
    const double w = weights[r];
    if (!(w > 0)) continue;
    ll += w * out_logl[r];
    for (int e = 0; e < E; e++) {
      out_num_acc[e] += w * out_num[(size_t)r * E + e];
      out_den_acc[e] += w * out_den[(size_t)r * E + e];
    }
  }
  *out_ll = ll;
}
}  // namespace

}  // namespace colate

extern "C" int colate_em_interval_calls_host(int R, int E, const int* kinds, const double* age_begin, const double* age_end,
                                             const double* epochs, const double* rates, const double* weights,
                                             double* out_num, double* out_den, double* out_logl, int* out_flags,
                                             double* out_num_acc, double* out_den_acc, double* out_ll, int math) {
  using namespace colate;
  if (math != 0 && math != 1) return fail(COLATE_EINVAL, "math must be 0 (<cmath>) or 1 (em_math)");
  if (int rc = check_interval_calls(R, E, kinds, age_begin, age_end, epochs, rates, weights, out_num, out_den, out_logl,
                                    out_flags, out_num_acc, out_den_acc, out_ll))
    return rc;
  if (math == 0)
    run_calls(em_interval::LibmMath{}, R, E, kinds, age_begin, age_end, epochs, rates, weights, out_num, out_den, out_logl,
              out_flags, out_num_acc, out_den_acc, out_ll);
  else
    run_calls(em_interval::EmMath{em::kExpTableHost}, R, E, kinds, age_begin, age_end, epochs, rates, weights, out_num,
              out_den, out_logl, out_flags, out_num_acc, out_den_acc, out_ll);
  return COLATE_OK;
}

extern "C" int colate_em_interval_batch_host(int B, int R, int E, const int* kinds, const double* age_begin,
                                             const double* age_end, const double* weights, const double* epochs,
                                             const double* init_rates, int max_iter, int min_iter, double rel_tol,
                                             double rate_floor, double* out_rates, int* out_iters, double* out_loglik,
                                             int* out_flags, int math) {
  using namespace colate;
  if (math != 0 && math != 1) return fail(COLATE_EINVAL, "math must be 0 (<cmath>) or 1 (em_math)");
  if (int rc = check_interval_batch(B, R, E, kinds, age_begin, age_end, weights, epochs, init_rates, max_iter, min_iter,
                                    rel_tol, rate_floor, out_rates, out_iters, out_loglik, out_flags))
    return rc;
  if (math == 0)
    run_fit(em_interval::LibmMath{}, B, R, E, kinds, age_begin, age_end, weights, epochs, init_rates, max_iter, min_iter,
            rel_tol, rate_floor, out_rates, out_iters, out_loglik, out_flags);
  else
    run_fit(em_interval::EmMath{em::kExpTableHost}, B, R, E, kinds, age_begin, age_end, weights, epochs, init_rates,
            max_iter, min_iter, rel_tol, rate_floor, out_rates, out_iters, out_loglik, out_flags);
  return COLATE_OK;
}

extern "C" int colate_bootstrap_rows_host(int B, int nb, int R, const double* block_weights, const double* tables, double* W) {
  using namespace colate;
  if (int rc = check_bootstrap_rows(B, nb, R, block_weights, tables)) return rc;
  if (!W) return fail(COLATE_EINVAL, "NULL pointer argument");
  std::vector<double> sums((size_t)B * R);  // (a refused call leaves W alone)
  bootstrap_rows(B, nb, R, block_weights, tables, sums.data());
  if (int rc = check_rows_finite(B, R, sums.data())) return rc;
  std::memcpy(W, sums.data(), sums.size() * sizeof(double));
  return COLATE_OK;
}

extern "C" int colate_bootstrap_em_interval_batch_host(int B, int nb, int R, int E, const int* kinds, const double* age_begin,
                                                       const double* age_end, const double* block_weights,
                                                       const double* tables, const double* epochs, const double* init_rates,
                                                       int max_iter, int min_iter, double rel_tol, double rate_floor,
                                                       double* out_rates, int* out_iters, double* out_loglik,
                                                       int* out_flags, int math) {
  using namespace colate;
  if (math != 0 && math != 1) return fail(COLATE_EINVAL, "math must be 0 (<cmath>) or 1 (em_math)");
  if (int rc = check_bootstrap_interval_batch(B, nb, R, E, kinds, age_begin, age_end, block_weights, tables, epochs, init_rates,
                                              max_iter, min_iter, rel_tol, rate_floor, out_rates, out_iters, out_loglik,
                                              out_flags))
    return rc;
  std::vector<double> W((size_t)B * R);
  bootstrap_rows(B, nb, R, block_weights, tables, W.data());
  if (math == 0)
    run_fit(em_interval::LibmMath{}, B, R, E, kinds, age_begin, age_end, W.data(), epochs, init_rates, max_iter, min_iter,
            rel_tol, rate_floor, out_rates, out_iters, out_loglik, out_flags);
  else
    run_fit(em_interval::EmMath{em::kExpTableHost}, B, R, E, kinds, age_begin, age_end, W.data(), epochs, init_rates,
            max_iter, min_iter, rel_tol, rate_floor, out_rates, out_iters, out_loglik, out_flags);
  return COLATE_OK;
}
