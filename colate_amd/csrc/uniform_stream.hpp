// colate_amd/csrc/uniform_stream.hpp -- the uniform stream of a `--seed` as every table fill forms it (the engine of `--pairs`,
// mut_pairs.cpp; the fill of `--samples`, fill_samples.cpp and fill_samples_kernel.hip): std::mt19937's words in bulk, two words
// to a double as std::uniform_real_distribution<double>(0, 1) turns them, and the check of both against this machine's library.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <random>
#include <sstream>

namespace colate_drv {

// std::mt19937's recurrence with the state regenerated 624 words at a time in loops the compiler vectorises (the library's
// operator() does the same work word by word: 7.5 ns per word on the build container, against ~2 here).  Same sequence by
// construction; bulk_stream_ok checks it against the library's generator before it is trusted.  State goes in and out of a
// std::mt19937 through its textual form (the 624 words and the position, [rand.eng.mers]).
class BulkMt19937 {
 public:
  bool load(const std::mt19937& g) {
    std::ostringstream os;
    os << g;
    std::istringstream is(os.str());
    for (int i = 0; i < 624; i++)
      if (!(is >> x_[i])) return false;
    if (!(is >> p_) || p_ > 624) return false;
    return true;
  }
  bool store(std::mt19937& g) const {
    std::ostringstream os;
    for (int i = 0; i < 624; i++) os << x_[i] << ' ';
    os << p_;
    std::istringstream is(os.str());
    return static_cast<bool>(is >> g);
  }
  // the next n 32-bit outputs
  void generate(uint32_t* out, size_t n) {
    while (n) {
      if (p_ >= 624) twist();
      const size_t k = std::min(n, (size_t)(624 - p_));
      const uint32_t* x = x_ + p_;
      for (size_t i = 0; i < k; i++) {  // tempering
        uint32_t y = x[i];
        y ^= y >> 11;
        y ^= (y << 7) & 0x9d2c5680u;
        y ^= (y << 15) & 0xefc60000u;
        y ^= y >> 18;
        out[i] = y;
      }
      out += k, n -= k, p_ += (uint32_t)k;
    }
  }
  // the same position as discard(n), without forming the outputs on the way (tempering is no part of the state)
  void skip(unsigned long long n) {
    while (n) {
      if (p_ >= 624) twist();
      const unsigned long long k = std::min<unsigned long long>(n, 624 - p_);
      p_ += (uint32_t)k, n -= k;
    }
  }
  void discard(unsigned long long n) {
    uint32_t tmp[624];
    while (n) {
      const size_t k = (size_t)std::min<unsigned long long>(n, 624);
      generate(tmp, k);
      n -= k;
    }
  }

 private:
  static uint32_t mix(uint32_t a, uint32_t b) {
    const uint32_t y = (a & 0x80000000u) | (b & 0x7fffffffu);
    return (y >> 1) ^ ((y & 1u) ? 0x9908b0dfu : 0u);
  }
  void twist() {
    for (int i = 0; i < 227; i++) x_[i] = x_[i + 397] ^ mix(x_[i], x_[i + 1]);          // (old words only)
    for (int i = 227; i < 454; i++) x_[i] = x_[i - 227] ^ mix(x_[i], x_[i + 1]);        // (new words of the first loop)
    for (int i = 454; i < 623; i++) x_[i] = x_[i - 227] ^ mix(x_[i], x_[i + 1]);        // (new words of the second)
    x_[623] = x_[396] ^ mix(x_[623], x_[0]);
    p_ = 0;
  }
  uint32_t x_[624];
  uint32_t p_ = 624;
};

// std::uniform_real_distribution<double>(0, 1) on std::mt19937 = generate_canonical<double, 53>: two 32-bit draws per value
// (libstdc++ bits/random.tcc)
inline double canonical_from_words(uint32_t r1, uint32_t r2) {
  double ret = ((double)r1 + (double)r2 * 4294967296.0) * 0x1p-64;
  if (ret >= 1.0) ret = std::nextafter(1.0, 0.0);
  return ret;
}

// does the bulk generator reproduce this machine's library on this seed?  (the sequence is part of the result)
inline bool bulk_stream_ok(unsigned seed) {
  std::mt19937 lib(seed);
  BulkMt19937 b;
  if (!b.load(lib)) return false;
  std::uniform_real_distribution<double> d(0, 1);
  uint32_t w[2 * 1300];
  b.generate(w, 2 * 1300);  // (across two regenerations of the state)
  for (int i = 0; i < 1300; i++)
    if (d(lib) != canonical_from_words(w[2 * i], w[2 * i + 1])) return false;
  std::mt19937 back;
  return b.store(back) && back == lib;
}

}  // namespace colate_drv
