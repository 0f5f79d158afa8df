// colate_amd/csrc/fill_device.h -- the age sampling of the table fill on the GPU (internal to libcolate_amd.so).
//
// Reference: include/coal/coal.cpp:2260-2273, 2279-2295 -- for every SNP a pair uses, 100 ages are drawn uniformly between the
// mutation's lower and upper age and the SNP's weight is added to the age bin of each of them, in the (pair, genome block)'s tables
// of shared / not-shared counts.  csrc/mut_pairs.cpp does that on the host (Engine::sample); this is the same arithmetic on the
// device, bit for bit:
//   * the uniforms of a --seed are ONE stream, the same for every pair: uploaded once, addressed by offset;
//   * a sample's age is u * span + begin by a separate multiply and add (no contraction), its bin the number of grid steps at or below
//     it, counted against both edges of the host's guard bands around the located steps (FastBin): where the two counts differ the
//     sample lies within 64 ulps of a step, the library expression would have to decide, and the pair is handed back to the host;
//   * the additions to one bin are a chain -- the same addend, one addition after the other, SNP after SNP --, and the chains of
//     different bins and different (pair, block) tables are independent: a wave per (pair, block), its bins in its lanes (the tables
//     live in registers), the counts of a SNP's samples per bin from an LDS histogram (integers: no order), then as many additions
//     as the fullest bin got, every lane on its own bins.
// Two ways in, one kernel (fill_kernel.hip): DeviceFill, for records and jobs staged from the host (the engine of `--pairs`,
// mut_pairs.cpp), and fill_sample_launch, for records and jobs the pair walk formed on the device (`--samples`,
// fill_samples_kernel.hip).  The guard bands come from FastBin (age_bins.hpp), the uniforms from uniform_stream.hpp.  No HIP type
// outside the __HIPCC__ part: host-only translation units include this.
#pragma once
#include <cstddef>
#include <cstdint>
#include <memory>
#include <string>
#include <vector>

namespace colate_drv {

struct FillRec {  // one used SNP (coal.cpp:2245-2297): the sampled range and what a sample adds
  float begin, end;    // age_begin (already clamped to the sample age 0), age_end; begin <= 0: the F path (not-shared weight only, no redraws)
  double w_sh, w_ns;   // f_DAF_target * DAF_ref / (N_ref * 100) and the same with f_AAF_target, as the host computes them
};
static_assert(sizeof(FillRec) == 24, "FillRec");

struct FillJob {        // the SNPs of one (pair, genome block), in file order
  uint64_t rec_off;     // first record, in the batch's staging buffer
  uint64_t u_off;       // stream offset of the first SNP's first uniform (SNP i: u_off + 100 i)
  uint32_t nrec;
  uint32_t table;       // which [2][A] table (shared | not shared) on the device
};

// The device side of the engine's fill (`--pairs` and a single pair): records and jobs staged from the host, batch by batch.
// Two page-locked staging buffers on the host (one is filled while the other is copied) and four record buffers on the device,
// each with a stream of its own, so that several launches run at the same time; the uniforms go up on a copy stream beside them.
// The implementation is in fill_kernel.hip; a build without device code defines the two free functions below to say so.
class DeviceFill {
 public:
  virtual ~DeviceFill() = default;
  // the two page-locked record buffers and their device copies (the slow part of the set-up -- gigabytes to lock --: callable from
  // another thread while uniforms are uploaded; before the first staging() / submit())
  virtual bool alloc_staging() = 0;
  // room for the uniform stream (known once the inputs have been read: a pair takes at most 100 per row)
  virtual bool alloc_uniforms(uint64_t max_uniforms) = 0;
  virtual FillRec* staging() = 0;  // pinned: where the next batch's records go
  virtual size_t staging_capacity() const = 0;
  // page-locks a host buffer the uniforms will be uploaded from (the ring of the stream's producer): pageable memory goes through
  // a staging copy at a few GB/s, 6 GB of uniforms are then seconds of wall time.  Failure is not an error (the upload works either way).
  virtual void pin(void* p, size_t bytes) = 0;
  // uniforms [off, off + n) of the stream: the copy is enqueued (launches submitted later wait for it on the device); the source may
  // be reused after sync_uploads()
  virtual bool upload_uniforms(uint64_t off, const double* src, size_t n) = 0;
  virtual bool sync_uploads() = 0;
  // records staging()[0 .. nrecs) and the jobs that refer to them: copied and launched asynchronously; staging() is another buffer afterwards
  virtual bool submit(const std::vector<FillJob>& jobs, size_t nrecs) = 0;
  // waits for everything; tables [max_tables][2][A]; flags per table: 1 = a sample needs the host (guard band, redraw, range): redo the pair
  virtual bool finish(std::vector<double>& tables, std::vector<int>& flags) = 0;
  const std::string& error() const { return err_; }
  double gpu_seconds() const { return gpu_s_; }

 protected:
  bool fail(const std::string& what, int) {
    err_ = what;
    return false;
  }
  double gpu_s_ = 0;

 private:
  std::string err_;
};

bool fill_device_available();  // a HIP device is there
// null (and a reason in `why`) when there is no device to use
std::unique_ptr<DeviceFill> make_device_fill(int device, int A, const double* guard_lo, const double* guard_hi, size_t max_tables,
                                             size_t batch_recs, std::string& why);

}  // namespace colate_drv

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
namespace colate_drv {
// The same kernel on jobs and records that already lie on the device (csrc/fill_samples_kernel.hip forms them there): device
// pointers throughout; U: the seed's uniform stream; g_lo / g_hi [A + 2]: the guard bands; tables [njobs][2][A] and flags [njobs]
// are zeroed by the caller.  Asynchronous on `stream`.
hipError_t fill_sample_launch(const FillJob* jobs, int njobs, const FillRec* recs, const double* U, const double* g_lo,
                              const double* g_hi, int A, double* tables, int* flags, hipStream_t stream);
}  // namespace colate_drv
#endif
