// colate_amd/csrc/em_interval.hpp
//
// coal_EM::EM_shared / EM_notshared of the reference (include/coal/coal_EM.cpp:153-468) for a mutation whose age is
// uniform on its branch [age_begin, age_end], and for age_begin == age_end, restated operand for operand and in the
// reference's order -- once, for the host and for gfx950 (em_interval_kernel.hip).  Build with -ffp-contract=off: a
// fused multiply-add anywhere in here changes the doubles.
//
// The formulas cancel heavily ((age_end - t_b - 1/l) + (t_e - age_end + 1/l) exp(..), term1 + exp(..) term2, the
// tmp < 0 -> log 0 branch); nothing is rearranged.  What IS rearranged is the control flow, so that a wave can share
// the work of one call among its lanes without changing a single operation or the order of any sum:
//
//   * get_tint (coal_EM.cpp:60-95) merges the two ages into the epoch grid.  The merged grid is never stored: with
//     eb / ee the epochs that hold age_begin / age_end (Call::eb, ee), its entries are epochs[0..eb], age_begin,
//     epochs[eb+1..ee], age_end, epochs[ee+1..], and the piece of epoch e between the ages is [lo(e), hi(e)].
//   * the cumulative rate over the merged grid is a left-to-right sum.  step_product() gives each addend (any lane),
//     cum_fold() adds them in the reference's order (one lane): a tree scan would re-associate the sum.
//   * log_values() gives num[e] / denom[e] in log space for one epoch (any lane): coal_EM.cpp:186-252, 323-431.
//   * normaliser() is the left-to-right logsumexp fold with its 1.0 sentinel (one lane): :254-258, 420-431.
//   * exp_at(), integ_fold(), finish_at(): the closing recurrence (:263-293, 435-466) split into its per-epoch
//     parts (any lane) and the running `integ` (one lane).
//
// call() runs these in order on the host; the kernel runs the same functions with epochs strided over the lanes.
//
// exp / log / log1p come from the template parameter M: LibmMath (<cmath>: the host twin that equals the reference
// bit for bit, it runs the same operations on the same libm) or EmMath (em_math.hpp: em_exp_t / em_log, bit-identical
// on gfx950 and on the host, so the device equals the second host twin bit for bit).
#pragma once
#include <cmath>

#include "em_math.hpp"

namespace em_interval {

struct LibmMath {
  double exp(double x) const { return std::exp(x); }
  double log(double x) const { return std::log(x); }
  double log1p(double x) const { return std::log1p(x); }
};

struct EmMath {
  const double* tab;  // em::kExpTableHost, or the kernel's copy of em::kExpTableDevice
  EM_HD double exp(double x) const {
    if (x != x) return x;  // (em_exp_t drops a NaN; libm hands it on, and so does the reference)
    return em::em_exp_t(x, tab);
  }
  EM_HD double log(double x) const { return em::em_log(x); }
  // log(1 + x) for x >= -1 from em_log: with u = fl(1 + x), log(u) * x / (u - 1) corrects for the rounding of u
  EM_HD double log1p(double x) const {
    const double u = 1.0 + x;
    if (u == 1.0) return x;
    if (!(u > 0.0)) return em::em_log(u);  // log1p(-1) = -inf
    return em::em_log(u) * x / (u - 1.0);
  }
};

EM_HD double log_zero() { return -__builtin_inf(); }
EM_HD bool inf_or_nan(double x) { return !(__builtin_fabs(x) <= 0x1.fffffffffffffp+1023); }

// coal_EM.cpp:5-31
template <class M>
EM_HD double logsumexp(const M& m, double loga, double logb) {
  if (inf_or_nan(loga)) return inf_or_nan(logb) ? log_zero() : logb;
  if (inf_or_nan(logb)) return loga;
  if (loga > logb) return loga + m.log1p(m.exp(logb - loga));
  return logb + m.log1p(m.exp(loga - logb));
}

// coal_EM.cpp:33-58
template <class M>
EM_HD double logminusexp(const M& m, double loga, double logb) {
  if (inf_or_nan(loga)) return log_zero();
  if (inf_or_nan(logb)) return loga;
  if (loga < logb) return log_zero();
  return loga + m.log1p(-m.exp(logb - loga));
}

// ---- A_ep / B_ep of the plain epoch grid (get_AB, coal_EM.cpp:97-151) ----
// cum[e]: cumulative rate at epochs[e], summed left to right (one lane)
EM_HD void ab_prefix(int E, const double* ep, const double* rt, double* cum) {
  cum[0] = 0.0;
  for (int i = 1; i < E; i++) cum[i] = cum[i - 1] + rt[i - 1] * (ep[i] - ep[i - 1]);
}
template <class M>
EM_HD void ab_at(const M& m, int E, const double* ep, const double* rt, const double* cum, int e, double* A, double* B) {
  const double rate = rt[e];
  double a = log_zero(), b = log_zero();
  if (e < E - 1) {
    const double t_begin = ep[e], t_end = ep[e + 1], inv = 1.0 / rate;
    if (rate > 0 && t_end != 0 && t_end - t_begin > 0) {
      a = logminusexp(m, -cum[e], -cum[e + 1]);
      b = (t_begin + inv) - (t_end + inv) * m.exp(-cum[e + 1] + cum[e]);
      b = m.log(b) - cum[e];
    }
  } else if (rate > 0) {
    a = -cum[e];
    b = m.log(ep[e] + 1.0 / rate) - cum[e];
  }
  A[e] = a;
  B[e] = b;
}

struct View {  // one (epochs, rates) and what follows from it alone
  int E;
  const double *ep, *rt, *A, *B;
};

struct Call {
  int kind;        // 0 = shared, 1 = not shared
  double a0, a1;   // age_begin <= age_end
  int eb, ee;      // ep_index[i_begin], ep_index[i_end]: the last epoch that starts at or before the age
  bool point;      // age_begin == age_end ("times_identical")
  double csb, csa; // cumulative rate at age_begin / age_end (cum_fold)
};

// how many epochs start at or before `age`, minus one (get_tint places an age in front of the first later boundary)
EM_HD int epoch_of(int E, const double* ep, double age) {
  int n = 0;
  for (int e = 0; e < E; e++) n += (ep[e] <= age) ? 1 : 0;
  return n - 1;
}

// the merged-grid entry in front of epochs[e] (e >= 1), and the addend of the cumulative rate that leads to epochs[e]
EM_HD double before_epoch(const View& v, const Call& c, int e) {
  return (e - 1 == c.ee) ? c.a1 : (e - 1 == c.eb) ? c.a0 : v.ep[e - 1];
}
EM_HD double step_product(const View& v, const Call& c, int e) { return v.rt[e - 1] * (v.ep[e] - before_epoch(v, c, e)); }

// On entry cse[e] = step_product(e) for e >= 1; on return cse[e] = cumulative rate at epochs[e], and c.csb / c.csa
// those at the two ages: coal_EM.cpp:176-179 / 314-317, the same additions in the same order (one lane).
EM_HD void cum_fold(const View& v, Call& c, double* cse) {
  double cum = 0.0;
  cse[0] = 0.0;
  for (int e = 0; e < v.E; e++) {
    if (e > 0) {
      cum = cum + cse[e];
      cse[e] = cum;
    }
    double at = v.ep[e];
    if (e == c.eb) {
      cum = cum + v.rt[e] * (c.a0 - at);
      c.csb = cum;
      at = c.a0;
    }
    if (e == c.ee) {
      cum = cum + v.rt[e] * (c.a1 - at);
      c.csa = cum;
    }
  }
}

// the piece of epoch e (eb <= e <= ee) that lies between the two ages
struct Piece {
  double lo, hi, cs_lo, cs_hi;
};
EM_HD Piece piece_of(const View& v, const Call& c, const double* cse, int e) {
  Piece p;
  p.lo = (e == c.eb) ? c.a0 : v.ep[e];
  p.cs_lo = (e == c.eb) ? c.csb : cse[e];
  p.hi = (e == c.ee) ? c.a1 : v.ep[e + 1];
  p.cs_hi = (e == c.ee) ? c.csa : cse[e + 1];
  return p;
}

// denom of an interval piece from term1, term2 and the decay over the piece (coal_EM.cpp:222-231, 376-385)
template <class M>
EM_HD double interval_denom(const M& m, const Call& c, double term1, double term2, double decay, double inv, double cs_lo) {
  double tmp = term1;
  tmp += decay * term2;
  if (tmp < 0.0) return log_zero();
  tmp = m.log(tmp);
  tmp += m.log(c.a1) + m.log(inv) - cs_lo;
  return tmp - m.log(c.a1 - c.a0);
}

// num[e], denom[e] in log space, before the normaliser is taken off (any lane; needs cum_fold's results)
template <class M>
EM_HD void log_values(const M& m, const View& v, const Call& c, const double* cse, int e, double* num, double* den) {
  const double rate = v.rt[e], inv = 1.0 / rate;
  const double age_begin = c.a0, age_end = c.a1;
  double n = log_zero(), d = log_zero();
  if (c.kind == 0) {  // ---- shared: coal_EM.cpp:186-252
    if (e > c.ee) {
      n = 0.0, d = 0.0;  // (not reached by the reference's loop: the outputs stay 0)
    } else if (e < c.eb) {
      n = v.A[e], d = v.B[e];
    } else {
      if (!c.point && rate > 0) {  // :212-231
        const Piece p = piece_of(v, c, cse, e);
        const double t_begin = p.lo, t_end = p.hi;
        const double decay = m.exp(-p.cs_hi + p.cs_lo);
        n = m.log((age_end - t_begin - inv) + (t_end - age_end + inv) * decay) - p.cs_lo - m.log(age_end - age_begin);
        const double x_begin = t_begin / age_end, x_end = t_end / age_end;
        const double term1 = (x_begin * (age_end - t_begin) / inv + 1.0 - 2.0 * (x_begin + inv / age_end));
        const double term2 = (-x_end * (age_end - t_end) / inv - 1.0 + 2.0 * (x_end + inv / age_end));
        d = interval_denom(m, c, term1, term2, decay, inv, p.cs_lo);
      }
      if (e == c.eb) {  // the part of epoch eb below age_begin: :198-210, 244-252
        double num_e = log_zero(), denom_e = log_zero();
        if (rate > 0) {
          const double t_begin = v.ep[e], t_end = age_begin, cs_i = cse[e], cs_i1 = c.csb;
          num_e = logminusexp(m, -cs_i, -cs_i1);
          denom_e = m.log((t_begin + inv) / inv - (t_end + inv) / inv * m.exp(-cs_i1 + cs_i)) + m.log(inv) - cs_i;
        }
        if (c.point) {
          n = num_e, d = denom_e;
        } else {
          n = logsumexp(m, n, num_e);
          d = logsumexp(m, d, denom_e);
        }
      }
    }
  } else {  // ---- not shared: coal_EM.cpp:323-431
    if (e < c.eb) {
      n = 0.0, d = 0.0;  // (set by the closing pass: 0 and the epoch's length)
    } else if (e > c.ee) {
      n = v.A[e], d = v.B[e];
    } else {
      if (!c.point && rate > 0.0) {  // :369-385
        const Piece p = piece_of(v, c, cse, e);
        const double t_begin = p.lo, t_end = p.hi;
        const double decay = m.exp(-p.cs_hi + p.cs_lo);
        n = m.log((t_begin - age_begin + inv) + (age_begin - t_end - inv) * decay) - p.cs_lo - m.log(age_end - age_begin);
        const double x_begin = t_begin / age_end, x_end = t_end / age_end, x_age_begin = age_begin / age_end;
        const double term1 = (x_begin * (t_begin - age_begin) / inv + 2.0 * (x_begin + inv / age_end) - x_age_begin);
        const double term2 = (-x_end * (t_end - age_begin) / inv - 2.0 * (x_end + inv / age_end) + x_age_begin);
        d = interval_denom(m, c, term1, term2, decay, inv, p.cs_lo);
      }
      if (e == c.ee) {  // the part of epoch ee above age_end: :331-357, 392-418
        const double cs_i = c.csa;
        double num_c, denom_c;
        if (e != v.E - 1) {
          const double t_begin = age_end, t_end = v.ep[e + 1], cs_i1 = cse[e + 1];
          num_c = logminusexp(m, -cs_i, -cs_i1);
          denom_c = m.log((t_begin + inv) - (t_end + inv) * m.exp(-cs_i1 + cs_i)) - cs_i;
        } else {  // the open last epoch
          num_c = -cs_i;
          denom_c = m.log(age_end + inv) - cs_i;
        }
        if (c.point) {
          const bool live = rate > 0 || e == v.E - 1;  // (:352: the reference asserts rate > 0 in the last epoch)
          n = live ? num_c : log_zero();
          d = live ? denom_c : log_zero();
        } else if (rate > 0) {
          n = logsumexp(m, n, num_c);
          d = logsumexp(m, d, denom_c);
        } else {
          n = log_zero(), d = log_zero();
        }
      }
    }
  }
  num[e] = n;
  den[e] = d;
}

// The log-normaliser: logsumexp over the epochs the reference visits, left to right, starting from its 1.0 sentinel
// (coal_EM.cpp:183, 254-258; 321, 337-348, 420-431).  One lane.
template <class M>
EM_HD double normaliser(const M& m, const View& v, const Call& c, const double* num) {
  double nc = 1.0;
  const int first = c.kind == 0 ? 0 : c.eb;
  for (int e = first; e <= c.ee; e++) nc = (nc == 1.0) ? num[e] : logsumexp(m, nc, num[e]);
  if (c.kind == 1)
    for (int e = c.ee + 1; e < v.E; e++) nc = logsumexp(m, nc, num[e]);
  return nc;
}

// The closing pass (coal_EM.cpp:263-293, 435-466) visits epochs [first, stop) with the `integ` recurrence and, where
// `last`, the final epoch without it; the others are constants.
struct Closing {
  int first, stop;
  bool last;
};
EM_HD Closing closing_of(const View& v, const Call& c) {
  Closing k;
  if (c.kind == 0) {
    k.first = 0;
    k.stop = (v.E - 1 < c.ee + 1) ? v.E - 1 : c.ee + 1;
    k.last = c.ee == v.E - 1;
  } else {
    k.first = c.eb;
    k.stop = v.E - 1;
    k.last = true;
  }
  return k;
}
EM_HD bool in_closing(const View& v, const Closing& k, int e) { return (e >= k.first && e < k.stop) || (k.last && e == v.E - 1); }

// num[e] = exp(num[e] - nc), denom[e] = exp(denom[e] - nc) (any lane)
template <class M>
EM_HD void exp_at(const M& m, const View& v, const Closing& k, double nc, int e, double* num, double* den) {
  if (!in_closing(v, k, e)) return;
  double n = num[e], d = den[e];
  n -= nc;
  d -= nc;
  num[e] = m.exp(n);
  den[e] = m.exp(d);
}
// integ[e]: what is left of 1 after num[first..e] (one lane)
EM_HD void integ_fold(const Closing& k, const double* num, double* integ) {
  double left = 1.0;
  for (int e = k.first; e < k.stop; e++) {
    if (left > 0.0) left -= num[e];
    else left = 0.0;
    integ[e] = left;
  }
}
// denom[e] += -epochs[e] num[e] + (epochs[e+1] - epochs[e]) integ[e], clamped at 0; the constants elsewhere (any lane)
EM_HD void finish_at(const View& v, const Call& c, const Closing& k, const double* integ, int e, double* num, double* den) {
  if (e >= k.first && e < k.stop) {
    double d = den[e];
    d += -v.ep[e] * num[e] + (v.ep[e + 1] - v.ep[e]) * integ[e];
    if (d < 0.0) d = 0.0;
    den[e] = d;
  } else if (k.last && e == v.E - 1) {
    double d = den[e];
    d -= v.ep[e] * num[e];
    if (d < 0.0) d = 0.0;
    den[e] = d;
  } else if (c.kind == 1 && e < c.eb) {
    num[e] = 0.0;
    den[e] = v.ep[e + 1] - v.ep[e];
  } else {
    num[e] = 0.0;
    den[e] = 0.0;
  }
}

EM_HD Call make_call(const View& v, int kind, double age_begin, double age_end) {
  Call c;
  c.kind = kind, c.a0 = age_begin, c.a1 = age_end;
  c.eb = epoch_of(v.E, v.ep, age_begin), c.ee = epoch_of(v.E, v.ep, age_end);
  c.point = age_begin == age_end;
  c.csb = 0.0, c.csa = 0.0;
  return c;
}

// One call on the host: num[E], denom[E] and the return value of EM_shared / EM_notshared.  work: [E] doubles.
template <class M>
inline double call(const M& m, const View& v, int kind, double age_begin, double age_end, double* num, double* den,
                   double* work) {
  Call c = make_call(v, kind, age_begin, age_end);
  for (int e = 1; e < v.E; e++) work[e] = step_product(v, c, e);
  cum_fold(v, c, work);
  for (int e = 0; e < v.E; e++) log_values(m, v, c, work, e, num, den);
  double nc = normaliser(m, v, c, num);
  if (inf_or_nan(nc)) {  // coal_EM.cpp:288-292, 461-465
    for (int e = 0; e < v.E; e++) num[e] = 0.0, den[e] = 0.0;
    return 0.0;
  }
  const Closing k = closing_of(v, c);
  for (int e = 0; e < v.E; e++) exp_at(m, v, k, nc, e, num, den);
  integ_fold(k, num, work);
  for (int e = 0; e < v.E; e++) finish_at(v, c, k, work, e, num, den);
  return nc;
}

// NaN / negative sufficient statistics (coal.cpp:3711-3714), as colate_em_estep reports them
EM_HD int value_flags(double n, double d) {
  int f = 0;
  if (n != n || d != d) f |= 1;     // COLATE_FLAG_NAN
  if (n < 0.0 || d < 0.0) f |= 2;   // COLATE_FLAG_NEG
  return f;
}

}  // namespace em_interval
