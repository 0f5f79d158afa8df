// colate_amd/csrc/tools/fill_kernel_check.cpp -- drives the product's age-sampling kernel (fill_kernel.o, fill_device.h) through
// the DeviceFill API over a scripted case, for tests/test_gpu_fill_kernel.py.  No copy of the kernel: the object the library
// links is linked here, and the script reproduces the host's interleavings of uploads, syncs and submits.
//   fill_kernel_check CASE OUT
// CASE, little-endian:
//   int32 A | uint64 max_tables | uint64 batch_recs | uint64 max_uniforms | double guard_lo[A + 2] | double guard_hi[A + 2]
//   then ops, each a uint32 code:
//     1 UPLOAD  uint64 off, uint64 n, double u[n]        upload_uniforms(off, u, n) from a page-locked copy kept to the end
//     2 SYNC                                             sync_uploads()
//     3 SUBMIT  uint32 refuse, uint64 njobs, uint64 nrecs, FillRec recs[nrecs], FillJob jobs[njobs]
//               records into staging() (at most staging_capacity() of them), then submit(jobs, nrecs); refuse = 1: the call must
//               return false (and the script goes on)
//     4 FINISH                                           finish(): OUT = double tables[max_tables][2][A] | int32 flags[max_tables]
// Exit status: 0 done; 2 unreadable case or output; 3 an API call failed (its error() on stderr); 4 a refusal was not refused.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../fill_device.h"

using colate_drv::DeviceFill;
using colate_drv::FillJob;
using colate_drv::FillRec;
static_assert(sizeof(FillJob) == 24, "FillJob");

namespace {

struct Reader {
  FILE* f;
  bool ok = true;
  template <class T>
  T get() {
    T v{};
    if (fread(&v, sizeof v, 1, f) != 1) ok = false;
    return v;
  }
  template <class T>
  void get_n(T* p, size_t n) {
    if (n && fread(p, sizeof(T), n, f) != n) ok = false;
  }
};

int api_error(const char* what, const std::string& err) {
  fprintf(stderr, "fill_kernel_check: %s failed: %s\n", what, err.c_str());
  return 3;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) {
    fprintf(stderr, "usage: fill_kernel_check CASE OUT\n");
    return 2;
  }
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  Reader in{f};
  const int A = in.get<int32_t>();
  const uint64_t max_tables = in.get<uint64_t>(), batch_recs = in.get<uint64_t>(), max_uniforms = in.get<uint64_t>();
  if (!in.ok || A < 0 || A > 4096) return 2;
  std::vector<double> lo((size_t)A + 2), hi((size_t)A + 2);
  in.get_n(lo.data(), lo.size());
  in.get_n(hi.data(), hi.size());
  if (!in.ok) return 2;
  // (declared before the DeviceFill: its destructor unregisters the page-locked upload sources, which must still be there)
  std::vector<std::unique_ptr<std::vector<double>>> sources;
  std::string why;
  const std::unique_ptr<DeviceFill> dev = colate_drv::make_device_fill(0, A, lo.data(), hi.data(), max_tables, batch_recs, why);
  if (!dev) return api_error("create", why);
  if (!dev->alloc_staging()) return api_error("alloc_staging", dev->error());
  if (!dev->alloc_uniforms(max_uniforms)) return api_error("alloc_uniforms", dev->error());
  std::vector<FillRec> recs;
  std::vector<FillJob> jobs;
  for (;;) {
    const uint32_t op = in.get<uint32_t>();
    if (!in.ok) return 2;  // (a script ends with FINISH)
    if (op == 1) {
      const uint64_t off = in.get<uint64_t>(), n = in.get<uint64_t>();
      if (!in.ok || n > (uint64_t)1 << 28) return 2;
      sources.emplace_back(new std::vector<double>(n));
      in.get_n(sources.back()->data(), n);
      if (!in.ok) return 2;
      dev->pin(sources.back()->data(), n * sizeof(double));
      if (!dev->upload_uniforms(off, sources.back()->data(), n)) return api_error("upload_uniforms", dev->error());
    } else if (op == 2) {
      if (!dev->sync_uploads()) return api_error("sync_uploads", dev->error());
    } else if (op == 3) {
      const uint32_t refuse = in.get<uint32_t>();
      const uint64_t nj = in.get<uint64_t>(), nr = in.get<uint64_t>();
      if (!in.ok || nj > (uint64_t)1 << 20 || nr > (uint64_t)1 << 26) return 2;
      recs.resize(nr);
      jobs.resize(nj);
      in.get_n(recs.data(), nr);
      in.get_n(jobs.data(), nj);
      if (!in.ok) return 2;
      const size_t fit = nr < dev->staging_capacity() ? nr : dev->staging_capacity();
      std::memcpy(dev->staging(), recs.data(), fit * sizeof(FillRec));
      const bool ok = dev->submit(jobs, nr);
      if (refuse) {
        if (ok) {
          fprintf(stderr, "fill_kernel_check: submit of %llu records accepted (batch of %llu)\n", (unsigned long long)nr,
                  (unsigned long long)batch_recs);
          return 4;
        }
        fprintf(stderr, "fill_kernel_check: submit refused: %s\n", dev->error().c_str());
      } else if (!ok) {
        return api_error("submit", dev->error());
      }
    } else if (op == 4) {
      std::vector<double> tables;
      std::vector<int> flags;
      if (!dev->finish(tables, flags)) return api_error("finish", dev->error());
      FILE* o = fopen(argv[2], "wb");
      if (!o || fwrite(tables.data(), sizeof(double), tables.size(), o) != tables.size() ||
          fwrite(flags.data(), sizeof(int), flags.size(), o) != flags.size())
        return 2;
      fclose(o);
      fclose(f);
      return 0;
    } else {
      return 2;
    }
  }
}
