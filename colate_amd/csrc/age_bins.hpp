// colate_amd/csrc/age_bins.hpp -- the age bin of an age, as every table fill and the interval cells take it: the library expression
// of the reference (age_bin_index) and FastBin, its steps located once with the guard bands around them -- what the engine of
// `--pairs` classifies samples with (mut_pairs.cpp), what both device fills hand their kernel as thresholds, and what the host
// twin of `--samples` measures near_band against (fill_samples.cpp).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

namespace colate_drv {

inline int age_bin_index(double x, double C) {  // coal.cpp:2265, 2284
  const double v = std::round(std::log(10 * x) * C);
  if (!(v > -2e9)) return 0;  // log(0) = -inf: the reference's (int) cast yields INT_MIN -> max(0, .) = 0
  return std::max(0, (int)v + 1);
}

// ------------------------------------------------------------------ the age bin of a sampled age, without the logarithm
// bin(x) = max(0, (int)round(log(10 x) * C) + 1) (coal.cpp:2265, 2284) is a step function of x with one step per age bin.
// The steps are located once by bisection over the doubles ON THE LIBRARY EXPRESSION ITSELF (age_bin_index); a sample is
// then classified by a table on its leading bits and one or two comparisons.  The library expression may disagree with the
// exact mathematical step by the last bits of log(): any x within 64 ulps of a located step goes through the library
// expression instead (log's error, under one ulp of a value below 24, moves the step by fewer than 16 ulps of x), so the
// result equals age_bin_index(x) for every x, by construction and by the self-check in the constructor.
class FastBin {
 public:
  FastBin(int A, double C) : A_(A), C_(C), thr_(A + 2), lo_(A + 2), hi_(A + 2) {
    const double inf = std::numeric_limits<double>::infinity();
    thr_[0] = lo_[0] = hi_[0] = -inf;
    thr_[A + 1] = lo_[A + 1] = hi_[A + 1] = inf;
    for (int k = 1; k <= A; k++) {
      uint64_t a = bits(1e-300), b = bits(1e300);  // f(a) < k <= f(b)
      while (b - a > 1) {
        const uint64_t mid = a + (b - a) / 2;
        if (f(from_bits(mid)) >= k) b = mid; else a = mid;
      }
      thr_[k] = from_bits(b);
      lo_[k] = from_bits(b - 64);
      hi_[k] = from_bits(b + 64);
    }
    base_ = bits(thr_[1]) >> kShift;
    const uint64_t top = bits(thr_[A]) >> kShift;
    cell_.resize(top - base_ + 2);
    for (size_t c = 0; c < cell_.size(); c++) {
      const double edge = std::max(from_bits((base_ + c) << kShift), thr_[1]);
      cell_[c] = (uint16_t)std::min(f(edge), A);
    }
    // self-check on the steps, their neighbourhoods and random samples; a failure switches the table off
    ok_ = true;
    std::mt19937_64 g(99);
    for (int k = 1; k <= A && ok_; k++)
      for (int d = -200; d <= 200 && ok_; d++) ok_ = agrees(from_bits(bits(thr_[k]) + d));
    for (int i = 0; i < 200000 && ok_; i++)
      ok_ = agrees(std::exp(std::uniform_real_distribution<double>(std::log(0.01), std::log(2e7))(g)));
    ok_ = ok_ && agrees(0.0) && agrees(1e-310) && agrees(0.05) && agrees(1e9);
  }
  bool ok() const { return ok_; }
  int bins() const { return A_; }
  // lower / upper edge of the guard band around step k (k = 1 .. A; [0] = -inf, [A + 1] = +inf): bin(x) = #{k : hi(k) <= x} for
  // every x outside all bands
  const double* guard_lo() const { return lo_.data(); }
  const double* guard_hi() const { return hi_.data(); }
  // age_bin_index(x, C), with every value >= A returned as A
  int operator()(double x) const {
    if (!ok_) return std::min(f(x), A_);
    if (x < lo_[1]) return 0;
    if (x >= hi_[A_]) return A_;
    if (x < hi_[1]) return x < thr_[1] ? std::min(f(x), A_) : slow_or(x, 1);
    const size_t c = (size_t)((bits(x) >> kShift) - base_);
    const int k = cell_[c];
    if (x < hi_[k]) return std::min(f(x), A_);
    if (x < lo_[k + 1]) return k;
    if (x >= hi_[k + 1]) return std::min(k + 1, A_);
    return std::min(f(x), A_);
  }

 private:
  static constexpr int kShift = 46;  // 11 exponent bits + 6 leading mantissa bits: a cell spans a factor <= 1 + 1/64, a bin e^0.1
  static uint64_t bits(double x) {
    uint64_t u;
    std::memcpy(&u, &x, 8);
    return u;
  }
  static double from_bits(uint64_t u) {
    double x;
    std::memcpy(&x, &u, 8);
    return x;
  }
  int f(double x) const { return age_bin_index(x, C_); }
  int slow_or(double x, int k) const { return x >= hi_[k] ? k : std::min(f(x), A_); }
  bool agrees(double x) const {
    FastBin* self = const_cast<FastBin*>(this);
    const bool keep = self->ok_;
    self->ok_ = true;
    const int fast = (*this)(x);
    self->ok_ = keep;
    return fast == std::min(f(x), A_);
  }
  int A_;
  double C_;
  std::vector<double> thr_, lo_, hi_;
  std::vector<uint16_t> cell_;
  uint64_t base_ = 0;
  bool ok_ = false;
};

}  // namespace colate_drv
